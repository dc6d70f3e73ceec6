"""Preconditioned SLQ on the GPU: mfx_lowrank_apply, the MFX_OP_PRECOND kind under the plain matvec and the Krylov / PCG drivers,
and the log-determinant estimator built on them, each against a restatement in fp64 torch / NumPy on the CPU inside this file:
dense S = P^-1/2 (from the eigen-decomposition of P itself, not from the formula under test), dense S A S, slogdet, and torch
autograd through the dense expression.

Tolerances: fp64 build against the fp64 restatement 1e-9 forward, 1e-7 gradients; fp32 build value rtol
1e-4, gradients rtol 1e-3 with atol 1e-5 |g|_inf.  Forward bounds are relative to the largest entry of the restated array; gradient
bounds are elementwise, |got - want| <= rtol |want| + atol |want|_inf (fp64: rtol 1e-7, atol 1e-7 |want|_inf).
The existing test of mfx_precond_apply is fp64 only, so the fp32 low-rank apply takes a bound of its own arithmetic:
z = scale (v - L (M (L^T v))) is three nested sums of m = n + 2 r + 8 rounded operations in all (the 8: the scale, the subtraction and
the roundings of the intermediates to fp32).  The worst case is m u A with u = eps / 2 the unit round-off and
A = scale (|v| + |L| (|M| (|L|^T |v|))) the sum of absolute values; rounding errors of independent operations add like a random walk,
sqrt(m) u A in standard deviation, and eight standard deviations cover the largest of the ~1e5 entries a case compares:
    |z - z_ref| <= 8 sqrt(m) u A = 4 sqrt(n + 2 r + 8) eps A     (eps = 2^-23; inputs rounded to fp32 on both sides).
At n = 4099 that is 3e-5 A, an eighth of what one dropped element of a 4099-term sum costs on average (A / n), so a tail or bounds
slip in the projection shows in fp32 too."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib, arnoldi, cg, lanczos, low_rank
    from matfree_extensions.operators import CsrOp, DenseOp, PreconditionedOp, RbfGramOp, StencilOp
    from matfree_extensions.util import gp_util

DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
CPU = torch.device("cpu")


def cpu(t):
    return t.detach().to(device=CPU, dtype=F64)


def randn(shape, seed, dtype=F64):
    return torch.randn(shape, dtype=F64, generator=torch.Generator().manual_seed(seed)).to(dtype)


def close(got, want, rtol, what=""):
    """max |got - want| <= rtol max |want|, printed before it is asserted"""
    got, want = cpu(got), cpu(want)
    err, ref = float((got - want).abs().max()), float(want.abs().max())
    print(f"{what}: err {err:.3e} of {ref:.3e} (bound {rtol:.0e})")
    assert err <= rtol * max(ref, 1e-300), (what, err, ref)


def tols(dtype):
    """(forward, gradient rtol, gradient atol in units of |g|_inf) of the dtype"""
    return (1e-9, 1e-7, 1e-7) if dtype == F64 else (1e-4, 1e-3, 1e-5)


def grad_close(got, want, dtype, what=""):
    """elementwise |got - want| <= rtol |want| + atol |want|_inf (allclose semantics), the worst ratio printed before it is asserted"""
    got, want = cpu(got), cpu(want)
    _, rtol, afac = tols(dtype)
    ref = float(want.abs().max())
    err = (got - want).abs()
    allowed = rtol * want.abs() + afac * ref
    print(f"{what}: grad err {float(err.max()):.3e} of {ref:.3e}, worst err / allowed {float((err / allowed.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= allowed).all()), (what, float(err.max()), ref)


# ---- restatements -------------------------------------------------------------------------------------------------------
def dense_inv_sqrt(L, s):
    """P^-1/2 for P = s I + L L^T from the eigen-decomposition of P (fp64, CPU)"""
    n = L.shape[0]
    lam, U = torch.linalg.eigh(s * torch.eye(n, dtype=F64) + L @ L.t())
    return (U / lam.sqrt()) @ U.t()


def softplus(x):
    return torch.nn.functional.softplus(x)


def dense_gram(X, raw, kernel, eps, minval=0.0):
    """K(X, X) + noise I in the parametrisation of RbfGramOp (fp64 torch, differentiable with respect to raw and X)"""
    rl, rs, rn = raw
    Z = X / softplus(rl).reshape(-1)
    diff = Z[:, None, :] - Z[None, :, :]
    sq = (diff * diff).sum(-1)
    if kernel == "rbf":
        K = torch.exp(-0.5 * sq)
    else:
        r = torch.sqrt(5.0 * sq + eps)
        K = (1.0 + r + r * r / 3.0) * torch.exp(-r)
    return softplus(rs) * K + (minval + softplus(rn)) * torch.eye(X.shape[0], dtype=F64)


def slq_values(B, V, k):
    """per-probe |v|^2 e1^T log(T) e1, T the symmetrised Hessenberg matrix of k Arnoldi steps with full re-orthogonalisation
    (fp64 torch, differentiable with respect to B)"""
    out = []
    for v in V:
        nrm = v.norm()
        Q = [v / nrm]
        H = torch.zeros((k, k), dtype=F64)
        for i in range(k):
            w = B @ Q[i]
            Qm = torch.stack(Q)
            h = Qm @ w
            w = w - Qm.t() @ h
            h2 = Qm @ w
            w = w - Qm.t() @ h2
            h = h + h2
            col = torch.zeros(k, dtype=F64)
            col[: i + 1] = h
            if i + 1 < k:
                beta = w.norm()
                col[i + 1] = beta
                Q.append(w / beta)
            H = H + torch.outer(col, torch.nn.functional.one_hot(torch.tensor(i), k).to(F64))
        T = 0.5 * (H + H.t())
        lam, U = torch.linalg.eigh(T)
        out.append(nrm**2 * (U[0] ** 2 * torch.log(lam)).sum())
    return torch.stack(out)


# ---- 1. low-rank apply ------------------------------------------------------------------------------------------------------
def _lowrank(dtype, lt, mid, scale, V, out=None):
    lib, code = _lib.get(), _lib.dtype_code(dtype)
    r, n = lt.shape
    p = V.shape[0]
    need = int(lib.mfx_lowrank_workspace_bytes(code, n, r, p))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)  # exactly the queried size
    Z = torch.empty_like(V) if out is None else out
    _lib.check(lib.mfx_lowrank_apply(code, n, r, _lib.ptr(lt), _lib.ptr(mid), _lib.ptr(scale), _lib.ptr(V), n, _lib.ptr(Z), n, p,
                                     _lib.ptr(ws), need, _lib.stream_ptr(DEV)))
    return Z


LOWRANK_SHAPES = [(n, r) for n in (1, 63, 1003, 4099) for r in (1, 5, 33) if r <= n]


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n,r", LOWRANK_SHAPES)
def test_lowrank_apply_against_the_dense_expression(n, r, dtype):
    lt = (randn((r, n), 7 * n + r) / math.sqrt(n)).to(dtype)
    A = randn((r, r), n + r)
    mid = (A @ A.t() / r + torch.eye(r, dtype=F64)).to(dtype)
    mid = 0.5 * (mid + mid.t())
    scale = torch.tensor([0.37], dtype=dtype)
    Ld, Md, sd = cpu(lt).t(), cpu(mid), float(cpu(scale))
    eps = float(torch.finfo(dtype).eps)
    ltg, midg, scg = lt.to(DEV), mid.to(DEV), scale.to(DEV)
    rows = {}
    for p in (1, 3, 17, 65):
        V = randn((65, n), 3 * n + r, dtype)[:p].contiguous()
        Vd = cpu(V)
        want = sd * (Vd - ((Vd @ Ld) @ Md) @ Ld.t())
        Vg = V.to(DEV)
        Z = _lowrank(dtype, ltg, midg, scg, Vg)
        if dtype == F64:
            close(Z, want, 1e-9, f"n={n} r={r} p={p}")
        else:
            bound = 4 * math.sqrt(n + 2 * r + 8) * eps * sd * (Vd.abs() + ((Vd.abs() @ Ld.abs()) @ Md.abs()) @ Ld.abs().t())
            err = (cpu(Z) - want).abs()
            print(f"n={n} r={r} p={p}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= bound).all())
        inplace = Vg.clone()
        _lowrank(dtype, ltg, midg, scg, inplace, out=inplace)
        assert torch.equal(inplace, Z), "in place differs from out of place"
        rows[p] = Z
    # a probe's bits do not depend on the batch: the rows of the p = 65 call against the same vectors alone and in smaller batches
    for b in (0, 16, 17, 64):
        one = _lowrank(dtype, ltg, midg, scg, randn((65, n), 3 * n + r, dtype)[b : b + 1].contiguous().to(DEV))
        assert torch.equal(one[0], rows[65][b]), f"row {b} of 65 differs from the same vector at p = 1"
    assert torch.equal(rows[17], rows[65][:17]) and torch.equal(rows[3], rows[65][:3]) and torch.equal(rows[1], rows[65][:1])


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n,r,p", [(1003, 5, 3), (4099, 33, 17)])
def test_lowrank_apply_is_the_woodbury_solve_of_precond_apply(n, r, p, dtype):
    L = (randn((n, r), n + 2 * r) / math.sqrt(n)).to(dtype).to(DEV)
    pre = low_rank.Preconditioner(L)
    s = 0.3
    V = randn((p, n), 11, dtype).to(DEV)
    minv, sdev = pre.minv(s)
    Z = _lowrank(dtype, pre.lt, minv, (1.0 / sdev).contiguous(), V)
    want = pre(V, s)
    Ld, Vd = cpu(L), cpu(V)
    exact = torch.linalg.solve(s * torch.eye(n, dtype=F64) + Ld @ Ld.t(), Vd.t()).t()
    if dtype == F64:
        close(Z, want, 1e-9, "against mfx_precond_apply")
        close(Z, exact, 1e-9, "against the dense solve")
    else:  # both are within the bound of the exact expression (module docstring), so within twice that of each other
        Md = cpu(minv)
        bound = 4 * math.sqrt(n + 2 * r + 8) * float(torch.finfo(dtype).eps) / s * (Vd.abs() + ((Vd.abs() @ Ld.abs()) @ Md.abs()) @ Ld.abs().t())
        err = (cpu(Z) - cpu(want)).abs()
        print(f"n={n} r={r} p={p}: max err / (2 bound) {float((err / (2 * bound)).max()):.3f}")
        assert bool((err <= 2 * bound).all()) and bool(((cpu(Z) - exact).abs() <= bound).all())


# ---- 2. the operator under the plain matvec ------------------------------------------------------------------------------------
def _factor(n, r, seed):
    return randn((n, r), seed) / math.sqrt(n) * 1.5


def _ragged_csr(n, seed):
    """a ragged matrix: row i has 1 + (i * 7) % 11 entries, one row of 40; diagonal always stored"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        m = 40 if i == n // 2 else 1 + (i * 7) % 11
        c = set(rng.choice(n, size=m - 1, replace=False).tolist()) | {i}
        rows += [i] * len(c)
        cols += sorted(c)
    vals = rng.standard_normal(len(rows))
    return np.array(rows), np.array(cols), vals


def _inner_cases():
    yield "dense", 96, F64, None
    yield "csr", 257, F64, None
    for d in (2, 9, 20):
        for kernel in ("rbf", "matern52"):
            yield f"gram-{kernel}-d{d}", 515, F32 if d == 9 else F64, (d, kernel)
    yield "gram-rbf-d2-f32", 515, F32, (2, "rbf")
    yield "stencil", 63, F64, None


def _build(name, n, dtype, extra):
    """-> (native operator, leaf parameters on the GPU, fn(cpu leaves...) -> dense A in fp64, cpu leaves, names)"""
    if name == "dense":
        A0 = randn((n, n), 1)
        leaf = A0.to(dtype).to(DEV).requires_grad_(True)
        return DenseOp(), [leaf], lambda A: A, [cpu(leaf).requires_grad_(True)]
    if name == "csr":
        row, col, vals = _ragged_csr(n, 2)
        op, v, _ = CsrOp.from_coo(row, col, vals, n, DEV)
        leaf = v.to(dtype).requires_grad_(True)
        ri, ci = op.row.long().cpu(), op.col.long().cpu()

        def dense(vv):
            return torch.zeros((n, n), dtype=F64).index_put((ri, ci), vv, accumulate=True)

        return op, [leaf], dense, [cpu(leaf).requires_grad_(True)]
    if name == "stencil":
        ny, nx = 9, 7
        st = randn((3, 3), 3)
        op = StencilOp((ny, nx), st, form="heat", boundary="dirichlet")
        coef = (1.0 + 0.3 * randn((ny, nx), 4)).to(dtype)
        leaf = coef.to(DEV).requires_grad_(True)
        w = torch.flip(st, (0, 1))

        def dense(cf):  # coef o (correlation with the flipped stencil, zero padding)
            Sm = torch.zeros((ny * nx, ny * nx), dtype=F64)
            for rr in range(ny):
                for cc in range(nx):
                    for dr in (-1, 0, 1):
                        for dc in (-1, 0, 1):
                            r2, c2 = rr + dr, cc + dc
                            if 0 <= r2 < ny and 0 <= c2 < nx:
                                Sm[rr * nx + cc, r2 * nx + c2] += w[dr + 1, dc + 1]
            return cf.reshape(-1)[:, None] * Sm

        return op, [leaf], dense, [cpu(leaf).requires_grad_(True)]
    d, kernel = extra
    X = randn((n, d), 10 + d).to(dtype)
    raw = [randn((d,), 20 + d) * 0.2 + 1.0, torch.tensor(0.4, dtype=F64), torch.tensor(-1.0, dtype=F64)]
    Xg = X.to(DEV).requires_grad_(True)
    leaves = [q.to(dtype).to(DEV).requires_grad_(True) for q in raw]
    op = RbfGramOp(Xg, noise_minval=1e-3, precision="fp32", kernel=kernel)
    eps = float(torch.finfo(dtype).eps)

    def dense(rl, rs, rn, Xc):
        return dense_gram(Xc, (rl, rs, rn), kernel, eps, minval=1e-3)

    return op, [*leaves, Xg], dense, [*[cpu(q).requires_grad_(True) for q in leaves], cpu(Xg).requires_grad_(True)]


@pytest.mark.parametrize("batch", [1, 70])
@pytest.mark.parametrize("name,n,dtype,extra", list(_inner_cases()), ids=[c[0] for c in _inner_cases()])
def test_preconditioned_matvec_and_its_backward(name, n, dtype, extra, batch):
    op, leaves, dense, cleaves = _build(name, n, dtype, extra)
    L = _factor(n, 5, 77).to(dtype)
    s = 0.6
    pre = low_rank.Preconditioner(L.to(DEV))
    pop = PreconditionedOp(op, pre, torch.tensor(s, dtype=dtype, device=DEV))
    S = dense_inv_sqrt(cpu(L), s)
    V = randn((batch, n), 5, dtype)
    W = randn((batch, n), 6, dtype)
    params = leaves[:-1] if name.startswith("gram") else leaves  # X travels inside the operator
    y = pop(V.to(DEV), *params)
    B = S @ dense(*cleaves) @ S
    want = cpu(V) @ B.t()
    fwd, _, _ = tols(dtype)
    close(y, want, fwd, f"{name} apply")
    from matfree_extensions.operators import _ApplyFn

    yt = _ApplyFn.apply(pop, True, V.to(DEV), *pop.constrain(*params))
    close(yt, cpu(V) @ B, fwd, f"{name} transposed apply")
    (y * W.to(DEV)).sum().backward()
    (want * cpu(W)).sum().backward()
    for i, (g, c) in enumerate(zip(leaves, cleaves)):
        assert g.grad is not None, f"{name}: leaf {i} received no gradient"
        grad_close(g.grad, c.grad, dtype, f"{name} leaf {i} (batch {batch})")


# ---- 3. the Krylov and PCG drivers on the kind ----------------------------------------------------------------------------------
def _gram_problem(n, d, seed, dtype=F64, kernel="rbf"):
    X = randn((n, d), seed).to(dtype)
    raw = [randn((d,), seed + 1) * 0.2 + 0.9, torch.tensor(0.5, dtype=F64), torch.tensor(-1.2, dtype=F64)]
    return X, raw


def _driver_outputs(alg_name, opb, V):
    if alg_name == "hessenberg":
        Q, H, r, c = arnoldi.hessenberg(opb, 6, reortho="full")(V)
        return [Q, H, r, c]
    (basis, (diag, off)), (rem, beta) = lanczos.tridiag(opb, 6, reortho=alg_name)(V)
    return [basis, diag, off, rem, beta]


@pytest.mark.parametrize("alg", ["full", "none", "hessenberg"])
def test_drivers_on_the_kind_against_the_dense_operator(alg):
    n, d, p = 300, 3, 3
    L = _factor(n, 6, 31)
    s = 0.4
    S = dense_inv_sqrt(L, s)
    pre = low_rank.Preconditioner(L.to(DEV))
    V = randn((p, n), 8)
    V = (V / V.norm(dim=-1, keepdim=True)).to(DEV)
    results = []
    for seed in (40, 50):  # two inner operators of one shape: the second call must not replay the first one's graph
        X, raw = _gram_problem(n, d, seed)
        for _rep in range(3):  # (the second call with identical arguments is the one libmfx captures, the third replays it)
            leaves = [q.to(DEV).requires_grad_(True) for q in raw]
            Xg = X.to(DEV).requires_grad_(True)
            pop = PreconditionedOp(RbfGramOp(Xg, noise_minval=1e-3), pre, s)
            outs = _driver_outputs(alg, pop.bind(*leaves), V)
            cot = [randn(tuple(o.shape), 60 + i).to(DEV) for i, o in enumerate(outs)]
            sum((o * c).sum() for o, c in zip(outs, cot)).backward()
        cl = [q.clone().requires_grad_(True) for q in raw]
        Xc = X.clone().requires_grad_(True)
        B = S @ dense_gram(Xc, cl, "rbf", float(torch.finfo(F64).eps), minval=1e-3) @ S
        Bg = B.detach().to(DEV).requires_grad_(True)
        ref = _driver_outputs(alg, DenseOp().bind(Bg), V)
        sum((o * c).sum() for o, c in zip(ref, cot)).backward()
        for i, (o, r_) in enumerate(zip(outs, ref)):
            close(o, r_, 1e-9, f"{alg} seed {seed} output {i}")
        (B * cpu(Bg.grad)).sum().backward()  # the dense gradient chained through S A(theta) S
        for i, (g, c) in enumerate(zip([*leaves, Xg], [*cl, Xc])):
            grad_close(g.grad, c.grad, F64, f"{alg} seed {seed} leaf {i}")
        results.append([o.detach().clone() for o in outs])
    assert not torch.allclose(results[0][1], results[1][1], rtol=1e-3), "the second operator gave the first one's result"


def test_pcg_solve_on_the_kind():
    n, d = 300, 3
    L = _factor(n, 6, 31)
    s = 0.4
    S = dense_inv_sqrt(L, s)
    X, raw = _gram_problem(n, d, 40)
    pop = PreconditionedOp(RbfGramOp(X.to(DEV), noise_minval=1e-3), low_rank.Preconditioner(L.to(DEV)), s)
    B = S @ dense_gram(X, raw, "rbf", float(torch.finfo(F64).eps), minval=1e-3) @ S
    b = randn((2, n), 9)
    x, _info = cg.cg_fixed_step(n)(pop.bind(*[q.to(DEV) for q in raw]), b.to(DEV))
    close(x, torch.linalg.solve(B, b.t()).t(), 1e-9, "cg on S A S")


def _abi_precond(inner, pre, s, dtype, n):
    """an outer descriptor and its mfx_precond built by hand around a given inner descriptor (kept alive by the caller)"""
    mid, scale = pre.inv_sqrt(s)
    pc = _lib.Precond()
    pc.pc_inner = C.addressof(inner)
    pc.pc_lt, pc.pc_mid, pc.pc_scale, pc.pc_rank = pre.lt.data_ptr(), mid.data_ptr(), scale.data_ptr(), pre.rank
    desc = _lib.Operator()
    desc.kind, desc.dtype, desc.n, desc.ctx = _lib.OP_PRECOND, _lib.dtype_code(dtype), n, C.addressof(pc)
    return desc, (pc, mid, scale)


def test_a_captured_call_is_not_replayed_against_a_changed_inner_descriptor():
    """The outer descriptor, the mfx_precond, the workspace and every output buffer stay the SAME objects at the same addresses; only
    one field of the inner descriptor (the matrix pointer) changes in place.  Everything the driver key holds besides the inner
    descriptor's bytes is then identical, so a key without them would replay the launches captured for the first matrix."""
    lib = _lib.get()
    n, k, p = 200, 5, 2
    A1 = randn((n, n), 70)
    A1 = (A1 @ A1.t() / n + torch.eye(n, dtype=F64)).to(DEV)
    A2 = (A1 + torch.diag(torch.linspace(0.0, 2.0, n, dtype=F64)).to(DEV)).contiguous()
    pre = low_rank.Preconditioner(_factor(n, 4, 71).to(DEV))
    inner = DenseOp().descriptor((A1,), F64, n)
    desc, keep = _abi_precond(inner, pre, 0.5, F64, n)
    V = randn((p, n), 72)
    V = (V / V.norm(dim=-1, keepdim=True)).to(DEV)
    ws = torch.empty(int(lib.mfx_workspace_bytes(C.byref(desc), n, k, p)), dtype=torch.uint8, device=DEV)
    xs, al, be, vn = (torch.empty(sh, dtype=F64, device=DEV) for sh in ((p, k + 1, n), (p, k), (p, k), (p,)))

    def call():
        with _lib.busy(ws):
            _lib.check(lib.mfx_lanczos_forward(C.byref(desc), _lib.ptr(V), n, k, p, _lib.ptr(xs), _lib.ptr(al), _lib.ptr(be), _lib.ptr(vn),
                                               _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))
        torch.cuda.synchronize()
        return al.clone(), be.clone()

    first = call()
    cap0, rep0 = _lib.graph_stats()
    for _ in range(3):
        again = call()
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    cap1, rep1 = _lib.graph_stats()
    print(f"captured {cap1 - cap0}, replayed {rep1 - rep0}")
    assert rep1 > rep0, "the repeated call was never replayed from a graph: this test would show nothing"
    inner.dense_a = A2.data_ptr()  # the ONLY change
    second = call()
    S = dense_inv_sqrt(cpu(pre.lt).t(), 0.5)
    (_, (d1, _o1)), _ = lanczos.tridiag(DenseOp().bind((S @ cpu(A1) @ S).to(DEV)), k, reortho="none")(V)
    (_, (d2, _o2)), _ = lanczos.tridiag(DenseOp().bind((S @ cpu(A2) @ S).to(DEV)), k, reortho="none")(V)
    close(first[0], d1, 1e-9, "first inner operator")
    close(second[0], d2, 1e-9, "changed inner operator")
    assert float((cpu(d1) - cpu(d2)).abs().max()) > 1e-3


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("inner_kind", ["gram", "dense"])
def test_the_kind_runs_at_exactly_the_queried_workspace(inner_kind, dtype):
    """mfx_op_apply and mfx_op_vjp_params (70 rows: two passes of the sweep) on the kind with exactly mfx_workspace_bytes between two
    poisoned guard zones: guards untouched, results bit-equal to a run with a generous workspace, a short workspace refused."""
    lib = _lib.get()
    n, p, guard = 515, 70, 4096
    pre = low_rank.Preconditioner(_factor(n, 5, 80).to(dtype).to(DEV))
    if inner_kind == "gram":
        op = RbfGramOp(randn((n, 3), 81, dtype).to(DEV), noise_minval=1e-3, precision="fp32")
        cparams = op.constrain(*[torch.tensor(v, dtype=dtype, device=DEV) for v in (0.9, 0.4, -1.0)])
    else:
        op, cparams = DenseOp(), (randn((n, n), 82, dtype).to(DEV),)
    inner = op.descriptor(cparams, dtype, n)
    desc, keep = _abi_precond(inner, pre, 0.6, dtype, n)
    V, W = randn((p, n), 83, dtype).to(DEV), randn((p, n), 84, dtype).to(DEV)
    need = int(lib.mfx_workspace_bytes(C.byref(desc), n, 1, p))
    st = _lib.stream_ptr(DEV)

    def run(ws_ptr, nbytes):
        y = torch.full((p, n), 7.0, dtype=dtype, device=DEV)
        gs, grads = op.new_grads(*cparams)
        rc_a = lib.mfx_op_apply(C.byref(desc), _lib.ptr(V), n, _lib.ptr(y), n, p, 0, ws_ptr, nbytes, st)
        rc_g = lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(W), n, _lib.ptr(V), n, p, C.byref(gs), ws_ptr, nbytes, st)
        torch.cuda.synchronize()
        return rc_a, rc_g, y, grads

    roomy = torch.zeros(4 * need, dtype=torch.uint8, device=DEV)
    rc_a, rc_g, y0, g0 = run(_lib.ptr(roomy), roomy.numel())
    assert (rc_a, rc_g) == (0, 0), lib.mfx_last_error()
    for poison in (0x00, 0xFF):
        buf = torch.full((need + 2 * guard,), poison, dtype=torch.uint8, device=DEV)
        assert (buf.data_ptr() + guard) % 256 == 0
        rc_a, rc_g, y, g = run(C.c_void_p(buf.data_ptr() + guard), 255)
        assert (rc_a, rc_g) == (-4, -4) and bool((y == 7.0).all()) and bool((buf == poison).all()), "a short workspace must be refused before any launch"
        rc_a, rc_g, y, g = run(C.c_void_p(buf.data_ptr() + guard), need)
        assert (rc_a, rc_g) == (0, 0), lib.mfx_last_error()
        assert bool((buf[:guard] == poison).all()) and bool((buf[guard + need :] == poison).all()), "wrote outside the queried workspace"
        assert torch.equal(y, y0) and all(torch.equal(a, b) for a, b in zip(g, g0)), "the result depends on what the workspace held"


# ---- 4. exactness: explicit probes sqrt(n) e_i, k = n ------------------------------------------------------------------------------
def _exact_case(seed):
    n = 24
    Qm, _ = torch.linalg.qr(randn((n, n), seed))
    A = Qm @ torch.diag(torch.linspace(1.0, 3.0, n, dtype=F64)) @ Qm.t()
    A = 0.5 * (A + A.t())
    L = randn((n, 3), seed + 1) / 2
    return n, A, L, 0.7


def _smallest_beta(B, V, k):
    """the smallest off-diagonal of the k-step Lanczos recurrence with full re-orthogonalisation over the probes (fp64 NumPy)"""
    B, out = B.numpy(), np.inf
    for v in V.numpy():
        Q = [v / np.linalg.norm(v)]
        for i in range(k - 1):
            w = B @ Q[i]
            for _ in range(2):
                w = w - np.array(Q).T @ (np.array(Q) @ w)
            out = min(out, np.linalg.norm(w))
            Q.append(w / np.linalg.norm(w))
    return out


def test_all_unit_probes_at_full_depth_give_slogdet():
    for seed in (0, 1, 2, 3, 4, 5):
        n, A, L, s = _exact_case(seed)
        B = dense_inv_sqrt(L, s) @ A @ dense_inv_sqrt(L, s)
        probes = math.sqrt(n) * torch.eye(n, dtype=F64)
        beta = _smallest_beta(B, probes, n)
        print(f"seed {seed}: smallest beta {beta:.3e}")
        if beta > 1e-6:  # the condition on the input
            break
    else:
        raise AssertionError("no seed met the condition on the input")
    logdet = gp_util.krylov_logdet_slq_p(n, sample=lambda key: key, num_batches=1)
    P = low_rank.Preconditioner(L.to(DEV)).bind(torch.tensor(s, dtype=F64, device=DEV))
    value, info = logdet(DenseOp().bind(A.to(DEV)), probes.to(DEV), P=P)
    want = float(torch.linalg.slogdet(A)[1])
    print(f"krylov_logdet_slq_p {float(value):.12f}, slogdet {want:.12f}")
    assert abs(float(value) - want) <= 1e-8
    assert set(info) == {"std", "std_rel"}


# ---- 5. variance and depth on the 512-point input -----------------------------------------------------------------------------------
def _pivoted_cholesky(K, rank):
    """greedy pivoted partial Cholesky (fp64 NumPy): (n, rank)"""
    n = K.shape[0]
    d = np.diag(K).copy()
    Lm = np.zeros((n, rank))
    for j in range(rank):
        piv = int(np.argmax(d))
        Lm[:, j] = (K[:, piv] - Lm[:, :j] @ Lm[piv, :j]) / np.sqrt(d[piv])
        d = d - Lm[:, j] ** 2
        d[piv] = -np.inf
    return Lm


_TABLE = {}


def _table_input():
    if not _TABLE:
        rng = np.random.default_rng(0)
        X = rng.standard_normal((512, 2))
        sq = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
        K = np.exp(-0.5 * sq)
        A = K + 0.1 * np.eye(512)
        Lm = _pivoted_cholesky(K, 30)
        probes = rng.choice([-1.0, 1.0], size=(16, 512))
        A_t, L_t, V_t = torch.tensor(A), torch.tensor(Lm), torch.tensor(probes)
        S = dense_inv_sqrt(L_t, 0.1)
        P = 0.1 * torch.eye(512, dtype=F64) + L_t @ L_t.t()
        _TABLE.update(X=X, A=A_t, L=L_t, V=V_t, exact=float(torch.linalg.slogdet(A_t)[1]), logdet_p=float(torch.linalg.slogdet(P)[1]),
                      plain={k: slq_values(A_t, V_t, k).detach() for k in (5, 10)},
                      pre={k: slq_values(S @ A_t @ S, V_t, k).detach() for k in (5, 10)})
    return _TABLE


def test_the_restatement_reproduces_the_table():
    t = _table_input()
    assert abs(t["exact"] - (-1062.075)) < 5e-3
    for k, (perr, pstd, qerr, qstd) in {5: (87.9, 47.7, -0.172, 4.12), 10: (0.16, 32.2, -0.172, 4.12)}.items():
        plain, pre = t["plain"][k], t["pre"][k] + t["logdet_p"]
        got = (float(plain.mean()) - t["exact"], float(plain.std(unbiased=False)), float(pre.mean()) - t["exact"],
               float(pre.std(unbiased=False)))
        print(f"k={k}: plain {got[0]:+.3f} / {got[1]:.2f}, preconditioned {got[2]:+.3f} / {got[3]:.2f}")
        assert abs(got[0] - perr) < 0.06 and abs(got[1] - pstd) < 0.06 and abs(got[2] - qerr) < 2e-3 and abs(got[3] - qstd) < 6e-3


@pytest.mark.parametrize("dtype", [F32, F64])
def test_variance_and_depth_on_the_512_point_input(dtype):
    t = _table_input()
    X = torch.tensor(t["X"], dtype=dtype, device=DEV)
    inv_sp = lambda v: math.log(math.expm1(v))  # noqa: E731
    raw = [torch.tensor(inv_sp(v), dtype=dtype, device=DEV) for v in (1.0, 1.0, 0.1)]
    op = RbfGramOp(X, precision="fp32")
    A = op.bind(*raw)
    pre, info = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=30))(low_rank.without_noise(A), 512)
    assert bool(info["success"])
    P = pre.bind(torch.tensor(0.1, dtype=dtype, device=DEV))
    V = t["V"].to(dtype).to(DEV)
    B = PreconditionedOp(op, pre, P.s).bind(*raw)
    fwd = tols(dtype)[0]
    for k in (5, 10):
        plain = lanczos.integrand_spd(torch.log, k, A)(V)
        prec = lanczos.integrand_spd(torch.log, k, B)(V) + float(P.logdet())
        close(plain, t["plain"][k], fwd, f"plain per-probe values, k={k}")
        # the library's factor may pivot differently on ties, so its P differs: per-probe values are restated with ITS factor
        Lc = cpu(pre.lt).t()
        Sc = dense_inv_sqrt(Lc, 0.1)
        want = slq_values(Sc @ t["A"] @ Sc, t["V"], k).detach() + float(torch.linalg.slogdet(0.1 * torch.eye(512, dtype=F64) + Lc @ Lc.t())[1])
        close(prec, want, fwd, f"preconditioned per-probe values, k={k}")
        ps, qs = float(cpu(plain).std(unbiased=False)), float(cpu(prec).std(unbiased=False))
        print(f"k={k}: spread plain {ps:.2f}, preconditioned {qs:.2f}, ratio {ps / qs:.2f}")
        assert ps >= 3.0 * qs
    pm, qm = float(cpu(lanczos.integrand_spd(torch.log, 5, A)(V)).mean()), None
    logdet = gp_util.krylov_logdet_slq_p(5, sample=lambda key: key, num_batches=1)
    qm = float(logdet(A, V, P=P)[0])
    print(f"k=5: plain mean off by {pm - t['exact']:+.2f}, preconditioned by {qm - t['exact']:+.3f}")
    assert abs(qm - t["exact"]) <= 2.0 and abs(pm - t["exact"]) > 40.0


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------
def _logml(dtype, which, probes, X, y, raws):
    n, d = X.shape
    constrain = gp_util.constraint_greater_than(1e-4)
    m_fun, _ = gp_util.mean_constant(shape_out=())
    k_fun, _ = gp_util.kernel_scaled_rbf(shape_in=(d,), shape_out=())
    solve_p = cg.pcg_fixed_step(150)
    sample = lambda key: key  # noqa: E731  (explicit probes)
    if which == "pslq":
        logpdf = gp_util.logpdf_krylov_pslq(solve_p, gp_util.krylov_logdet_slq_p(8, sample=sample, num_batches=1))
    else:
        logpdf = gp_util.logpdf_krylov_p(solve_p, gp_util.krylov_logdet_slq(8, sample=sample, num_batches=1))
    precondition = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=20))
    lik, _ = gp_util.likelihood_pdf_p(gp_util.gram_matvec(precision="fp32"), logpdf, precondition, constrain=constrain)
    leaves = [q.to(dtype).to(DEV).requires_grad_(True) for q in raws]
    value, info = gp_util.target_logml(gp_util.model_gp(m_fun, k_fun), lik)(
        X.to(dtype).to(DEV), y.to(dtype).to(DEV), probes.to(dtype).to(DEV), params_mean={"constant_value": leaves[0]},
        params_kernel={"raw_lengthscale": leaves[1], "raw_outputscale": leaves[2]}, params_likelihood={"raw_noise": leaves[3]})
    grads = torch.autograd.grad(value, leaves)
    return value, grads, leaves


@pytest.mark.parametrize("dtype", [F32])
def test_log_marginal_likelihood_end_to_end(dtype):
    n, d, k = 600, 3, 8
    X = randn((n, d), 90)
    y = torch.sin(X.sum(-1)) + 0.1 * randn((n,), 91)
    raws = [torch.tensor(0.1, dtype=F64), randn((d,), 92) * 0.1 + 0.8, torch.tensor(0.3, dtype=F64), torch.tensor(-2.0, dtype=F64)]
    probes = torch.sign(randn((8, n), 93))
    value, grads, leaves = _logml(dtype, "pslq", probes, X, y, raws)
    # the restatement of the same estimator, P held constant: the factor the library built, as data
    with torch.no_grad():
        op = RbfGramOp(X.to(dtype).to(DEV), noise_minval=1e-4, precision="fp32")
        bound = op.bind(*leaves[1:])
        pre, _ = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=20))(low_rank.without_noise(bound), n)
    Lc = cpu(pre.lt).t()
    cl = [q.clone().requires_grad_(True) for q in raws]
    Xr = cpu(X.to(dtype))
    noise = float(1e-4 + softplus(cl[3]))
    S = dense_inv_sqrt(Lc, noise)
    A = dense_gram(Xr, (cl[1], cl[2], cl[3]), "rbf", 0.0, minval=1e-4)
    logdet = slq_values(S @ A @ S, cpu(probes.to(dtype)), k).mean() + torch.linalg.slogdet(noise * torch.eye(n, dtype=F64) + Lc @ Lc.t())[1]
    res = cpu(y.to(dtype)) - cl[0]
    want = -0.5 * logdet - 0.5 * res @ torch.linalg.solve(A, res) - n / 2 * math.log(2 * math.pi)
    wgrads = torch.autograd.grad(want, cl)
    fwd = tols(dtype)[0]
    print(f"logml {float(value):.8f}, restated {float(want):.8f}")
    assert abs(float(value) - float(want)) <= fwd * abs(float(want))
    for i, (g, w) in enumerate(zip(grads, wgrads)):
        grad_close(g, w, dtype, f"logml raw parameter {i}")
    # no gradient through P: the factor and the shift the preconditioner holds are detached
    assert not pre.lt.requires_grad


def test_the_unpreconditioned_call_is_unchanged_and_P_gets_no_gradient():
    """logpdf_krylov_p with krylov_logdet_slq: the same call twice gives the same bits, and they are the bits of the estimator
    assembled by hand from the pieces that call is documented to consist of (integrand_spd on the unpreconditioned operator, the
    PCG solve with P) -- the composition this change must leave alone."""
    n, d = 600, 3
    X = randn((n, d), 90)
    y = torch.sin(X.sum(-1)) + 0.1 * randn((n,), 91)
    raws = [torch.tensor(0.1, dtype=F64), randn((d,), 92) * 0.1 + 0.8, torch.tensor(0.3, dtype=F64), torch.tensor(-2.0, dtype=F64)]
    probes = torch.sign(randn((8, n), 93))
    v1, g1, leaves = _logml(F32, "plain", probes, X, y, raws)
    v2, g2, _ = _logml(F32, "plain", probes, X, y, raws)
    assert torch.equal(v1, v2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    Xg, yg = X.to(F32).to(DEV), y.to(F32).to(DEV)
    hand = [q.detach().clone().requires_grad_(True) for q in leaves]
    A = RbfGramOp(Xg, noise_minval=1e-4, precision="fp32").bind(hand[1], hand[2], hand[3])
    noise = gp_util.constraint_greater_than(1e-4)(hand[3])
    pre, _ = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=20))(low_rank.without_noise(A), n)
    P = pre.bind(noise)
    logdet = lanczos.integrand_spd(torch.log, 8, A)(probes.to(F32).to(DEV)).mean(dim=0) / 2
    mean = hand[0].expand(n)
    tmp, _ = cg.pcg_fixed_step(150)(A, yg - mean, P=P)
    value = -logdet - 0.5 * ((yg - mean) @ tmp) - n / 2 * math.log(2 * math.pi)
    assert torch.equal(value, v1)
    for a, b in zip(torch.autograd.grad(value, hand), g1):
        assert torch.equal(a, b)
    # P receives no gradient: the preconditioned estimator's value depends on the noise through A only
    s = torch.tensor(0.2, dtype=F32, device=DEV, requires_grad=True)
    pop = PreconditionedOp(A.op, pre, s)
    assert not pop.s.requires_grad and not pre.inv_sqrt(s)[0].requires_grad
    out = gp_util.krylov_logdet_slq_p(4, sample=lambda key: key, num_batches=1)(A, probes.to(F32).to(DEV), P=pre.bind(s))[0]
    out.backward()
    assert s.grad is None
