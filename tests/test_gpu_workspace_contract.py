"""The workspace contract of include/mfx.h: "every buffer is owned by the caller", sizes come from the mfx_*_workspace_bytes queries.

Every case runs one operation three ways --
  A: workspaces from tests/_guarded_ws.py, exactly the queried size between two guard bands, every byte 0x00;
  B: the same with every byte 0xFF (NaN as fp32 / fp64, -1 as an integer: data in memory the test owns);
  C: the ordinary ``_lib._take``
-- and asserts that the guard bands are untouched after A and B (no write outside the queried size), that every output and every
gradient of A is ``torch.equal`` to B's and finite (nothing read that was not written first), and that A equals C (the library has
no atomics and documents bit-reproducibility; C is the path the oracle tests pin).  The Krylov drivers are called three times per
poison on one guarded buffer, so that the hipGraph capture and replay of the call run on poisoned scratch too.

Strided outputs the case owns have a leading dimension beyond their width and a sentinel in the padding, which must survive.  A second
group goes through ctypes once per workspace-taking entry point: the queried size is accepted, and 255 bytes are refused with
MFX_ERR_WORKSPACE before anything is launched (outputs, workspace and guards untouched).

Shapes: n = 300 unless the branch needs n >= 2048; the tables name the kernel branch each row is there for."""

import contextlib
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _guarded_ws import GuardedWs
from matfree_extensions import _lib, arnoldi, cg, lanczos, low_rank
from matfree_extensions.operators import CallbackOp, CsrOp, DenseOp, RbfGramOp, RowShardedOp, _ApplyFn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
SENT = -77.0
F32, F64 = torch.float32, torch.float64
MFX_ERR_INVALID, MFX_ERR_WORKSPACE = -1, -4


# ---------------------------------------------------------------------------------------------------------------------------
# the three-way runner
# ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _installed(take):
    """``_lib._take`` replaced without pytest (the child process of the probe-group case)"""
    old, _lib._take = _lib._take, take
    try:
        yield
    finally:
        _lib._take = old


def _cpu(out):
    return {k: v.detach().cpu() for k, v in out.items()}


def _same(got, ref, what):
    assert set(got) == set(ref), what
    for key, r in ref.items():
        g = got[key]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, key)
        if not torch.equal(g, r):
            bad = ((g != r) | (g != g)).reshape(-1)
            diff = (g - r).abs().reshape(-1) if g.is_complex() else (g.double() - r.double()).abs().reshape(-1)
            known = diff[diff == diff]
            worst = float(known.max()) if known.numel() else float("nan")
            raise AssertionError(f"{what}: {key} differs in {int(bad.sum())} of {g.numel()} entries "
                                 f"(first at flat index {int(bad.nonzero()[0])}, max |diff| {worst})")


def _finite(got, what):
    for key, g in got.items():
        if g.is_floating_point() or g.is_complex():
            assert bool(torch.isfinite(g).all()), f"{what}: {key} is not finite"


class Contract:
    def __init__(self, install):
        self.install = install
        self.guard = GuardedWs(busy=_lib._ws_busy)
        self.guarded = False  # inside run(): the guarded allocator is installed

    def run(self, fn, what, repeats=1, uses_ws=True):
        """fn() -> {name: tensor}, the same computation on the same inputs every time"""
        ref = _cpu(fn())  # C
        _finite(ref, what + " [ordinary]")
        first = None
        with self.install(self.guard.take), self._flag():
            for poison in (0x00, 0xFF):
                self.guard.poison = poison
                for rep in range(repeats):
                    tag = f"{what} [poison 0x{poison:02X}, call {rep}]"
                    before = self.guard.handed_out
                    got = _cpu(fn())
                    self.guard.verify()
                    assert not uses_ws or self.guard.handed_out > before, tag + ": the call took no workspace from the guarded allocator"
                    _finite(got, tag)
                    if first is not None:
                        _same(got, first, tag + " against poison 0x00")
                    first = first or got
                    _same(got, ref, tag + " against the ordinary allocator")
        return ref

    @contextlib.contextmanager
    def _flag(self):
        self.guarded = True
        try:
            yield
        finally:
            self.guarded = False


@pytest.fixture
def contract(monkeypatch):
    @contextlib.contextmanager
    def install(take):
        with monkeypatch.context() as m:
            m.setattr(_lib, "_take", take)
            yield

    return Contract(install)


# ---------------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------------
def inv_softplus(v):
    return math.log(math.expm1(v))


def randn(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).to(dtype).to(DEV)


def gram(n, d, dtype, ard=False, kernel="rbf", precision="f16x3", xgrad=False):
    """-> (operator, [raw lengthscale, raw outputscale, raw noise] requiring grad); lengthscales ~ sqrt(d): kernel values of order 1"""
    X = randn((n, d), dtype, 7 * n + d)
    if xgrad:
        X.requires_grad_(True)
    base = 0.7 * math.sqrt(d)
    ls = [inv_softplus(base * (1.0 + 0.1 * (c % 5))) for c in range(d)] if ard else inv_softplus(base)
    raw = (ls, inv_softplus(0.8), -1.0)
    params = [torch.tensor(r, dtype=dtype, device=DEV, requires_grad=True) for r in raw]
    return RbfGramOp(X, noise_minval=1e-4, precision=precision, kernel=kernel), params


def dense(n, dtype):
    B = randn((n, n), torch.float64, 11 * n)
    A = (B @ B.T / n + 2.0 * torch.eye(n, dtype=torch.float64, device=DEV)).to(dtype)
    return DenseOp(), [A.requires_grad_(True)]


def csr(n, dtype):
    """a sparse matrix with one row of 100 entries (longer than the 64 a wave covers at once)"""
    rng = np.random.default_rng(n)
    rows, cols = [], []
    for i in range(n):
        c = {i, *rng.choice(n, size=100 if i == 7 else 5, replace=False).tolist()}
        rows += [i] * len(c)
        cols += sorted(c)
    vals = rng.standard_normal(len(rows)) + 3.0 * (np.array(rows) == np.array(cols))
    op, vt, _order = CsrOp.from_coo(rows, cols, vals, n, DEV)
    assert op.max_row_nnz > 64
    return op, [vt.to(dtype).requires_grad_(True)]


def weights(t):
    """a fixed cotangent of the shape of t"""
    w = torch.cos(torch.arange(t.numel(), device=t.device, dtype=torch.float64) * 0.37 + 0.1)
    return w.reshape(t.shape).to(t.dtype if not t.is_complex() else torch.float64)


def grads_of(outs, wrt):
    got = torch.autograd.grad(outs, wrt, [weights(t) for t in outs], allow_unused=True)
    return [torch.zeros(()) if g is None else g for g in got]


def named(prefix, tensors):
    return {f"{prefix}{i}": t for i, t in enumerate(tensors)}


# ---------------------------------------------------------------------------------------------------------------------------
# Gram operator: mfx_op_apply
# ---------------------------------------------------------------------------------------------------------------------------
MODES = ("fp32", "f16x3-matvec", "f16x3")
# (n, d, p, dtype, kernel, ard, branch)
APPLY = [
    (300, 3, 1, F32, "rbf", False, "VALU"),
    (300, 8, 5, F32, "rbf", False, "fat split kernel"),
    (300, 8, 5, F32, "matern32", False, "h3"),
    (300, 8, 65, F32, "rbf", False, "two probe chunks"),
    (2304, 4, 3, F32, "rbf", False, "1-3 vectors on matrix cores"),
    (300, 13, 8, F32, "rbf", False, "four distance MFMAs"),
    (300, 20, 8, F32, "rbf", False, "pre-packed DPAD 32"),
    (300, 50, 8, F32, "rbf", False, "exact fp32 matrix cores"),
    (300, 129, 8, F32, "rbf", False, "wide VALU"),
    (300, 3, 5, F64, "rbf", False, "fp64 VALU"),
    (300, 40, 5, F64, "matern52", True, "fp64 wide VALU"),
]
APPLY_CASES = [(*row, mode) for row in APPLY for mode in (MODES if row[3] == F32 else MODES[:1])]


@pytest.mark.parametrize("n,d,p,dtype,kernel,ard,branch,mode", APPLY_CASES,
                         ids=[f"{r[0]}-{r[1]}-{r[2]}-{'f32' if r[3] == F32 else 'f64'}-{r[4]}-{r[7]}" for r in APPLY_CASES])
def test_gram_apply(contract, n, d, p, dtype, kernel, ard, branch, mode):
    op, params = gram(n, d, dtype, ard=ard, kernel=kernel, precision=mode)
    V = randn((p, n), dtype, 3)

    def fn():
        with torch.no_grad():
            return {"y": op(V, *params)}

    contract.run(fn, f"mfx_op_apply {branch}")


@pytest.mark.parametrize("mode", MODES)
def test_gram_apply_row_block_with_padded_output(contract, mode):
    """rows [64, 164) of the (300, 8, 5) operator into a (p, ldy = 103) buffer: the padding of every output row survives"""
    n, d, p, row0, nrows = 300, 8, 5, 64, 100
    ldy = nrows + 3
    op, params = gram(n, d, F32, precision=mode)
    cparams = [q.detach() for q in op.constrain(*params)]
    V = randn((p, n), F32, 4)
    lib = _lib.get()

    def fn():
        desc = op.descriptor(cparams, F32, n)
        desc.row0, desc.nrows = row0, nrows
        ws = _lib.workspace(desc, n, 1, p, DEV)
        y = torch.full((p, ldy), SENT, dtype=F32, device=DEV)
        _lib.check(lib.mfx_op_apply(C.byref(desc), _lib.ptr(V), n, _lib.ptr(y), ldy, p, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))
        assert bool((y[:, nrows:] == SENT).all()), "mfx_op_apply wrote into the padding of y"
        return {"y": y[:, :nrows]}

    got = contract.run(fn, "mfx_op_apply row block")
    with torch.no_grad():
        whole = op(V, *params)[:, row0 : row0 + nrows].cpu()
    assert torch.allclose(got["y"], whole, rtol=1e-3, atol=1e-3)  # (a sanity check that these ARE rows 64.. of the operator)


# ---------------------------------------------------------------------------------------------------------------------------
# Gram operator: mfx_op_vjp_params through autograd (parameters, inputs X and the vectors)
# ---------------------------------------------------------------------------------------------------------------------------
VJP = [
    (700, 3, 33, F32, "split GEMM with hws"),
    (2304, 4, 3, F32, "split GEMM with hws, n >= 2048"),
    (300, 8, 5, F32, "VALU sweep"),
    (300, 20, 16, F32, "DPAD-32 sweep"),
    (300, 50, 16, F32, "DPAD-64 partials of 66 doubles"),
    (300, 129, 5, F32, "wide sweep with selections"),
    (300, 3, 5, F64, "fp64 sweep"),
    (300, 40, 5, F64, "fp64 wide sweep"),
]


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "scalar"])
@pytest.mark.parametrize("n,d,batch,dtype,branch", VJP, ids=[f"{r[0]}-{r[1]}-{r[2]}-{'f32' if r[3] == F32 else 'f64'}" for r in VJP])
def test_gram_vjp_params(contract, n, d, batch, dtype, branch, ard):
    op, params = gram(n, d, dtype, ard=ard, xgrad=True)
    V = randn((batch, n), dtype, 5).requires_grad_(True)

    def fn():
        y = op(V, *params)
        return {"y": y, **named("g", grads_of((y,), (V, *params, op.X)))}

    contract.run(fn, f"mfx_op_vjp_params {branch}")


# ---------------------------------------------------------------------------------------------------------------------------
# dense and CSR operators
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_dense_and_csr_operators(contract, kind, dtype):
    n, p = 300, 5
    op, params = (dense if kind == "dense" else csr)(n, dtype)
    V = randn((p, n), dtype, 6).requires_grad_(True)

    def fn():
        y = op(V, *params)
        yt = _ApplyFn.apply(op, True, V, *op.constrain(*params))
        return {"y": y, "yt": yt, **named("g", grads_of((y, yt), (V, *params)))}

    contract.run(fn, f"{kind} operator")


# ---------------------------------------------------------------------------------------------------------------------------
# Krylov drivers
# ---------------------------------------------------------------------------------------------------------------------------
def _krylov_fn(driver, reortho, op, params, V, k, contract, tally):
    """forward and adjoint of one driver; V requires grad or not (dv == NULL).  tally: {"forward" / "adjoint": [captures, replays]} of
    the calls made under the guarded allocator (mfx_graph_stats read around each direction)"""
    wrt = ([V] if V.requires_grad else []) + list(params)

    def count(direction, before):
        after = _lib.graph_stats()
        if contract.guarded:
            tally[direction][0] += after[0] - before[0]
            tally[direction][1] += after[1] - before[1]
        return after

    def fn():
        stats = _lib.graph_stats()
        if driver == "lanczos":
            (basis, (diag, off)), (q, b) = lanczos.tridiag(op, k, reortho=reortho)(V, *params)
            outs = (basis, diag, off, q, b)
        else:
            outs = arnoldi.hessenberg(op, k, reortho=reortho)(V, *params)
        stats = count("forward", stats)
        grads = grads_of(outs, wrt)
        count("adjoint", stats)
        return {**named("out", outs), **named("g", grads)}

    return fn


def _krylov_sweep(contract, opkind, dtype, ks=(1, 7), ps=(1, 5)):
    """Every run is six guarded calls (three per poison) on ONE workspace.  The graph key of a driver call holds the workspace pointer
    and every input, output and parameter pointer; the wrappers allocate the outputs and the constrained parameters afresh per call,
    so a replay needs torch's caching allocator to hand back the same addresses -- it does once the same call has run before (the
    ordinary-allocator run and the first guarded call come first), which is why EVERY run, in each direction, is asked for at least
    one replay on its poisoned workspace.  A capture is asked for once per driver and direction over the sweep, not per run:
    lanczos.tridiag(reortho="none") is mfx_lanczos_forward / _adjoint, the other three run mfx_arnoldi_forward / _adjoint, and the
    forward call of hessenberg(reortho="none") is the very call tridiag(reortho="full") made just before on the same buffers -- it
    replays that graph (0 captures, 6 replays)."""
    n = 300
    graphs = os.environ.get("MFX_GRAPHS") != "0"
    op, params = gram(n, 8, dtype) if opkind == "gram" else dense(n, dtype)
    captures = {(entry, direction): 0 for entry in ("lanczos", "arnoldi") for direction in ("forward", "adjoint")}
    for p in ps:
        V0 = randn((p, n), dtype, 8 + p)
        V0 = V0 / V0.norm(dim=-1, keepdim=True)
        for vgrad in (True, False):
            V = V0.clone().requires_grad_(vgrad)
            for k in ks:
                for driver in ("lanczos", "arnoldi"):
                    for reortho in ("none", "full"):
                        what = f"{driver} reortho={reortho} {opkind} k={k} p={p} dv={'yes' if vgrad else 'NULL'}"
                        tally = {"forward": [0, 0], "adjoint": [0, 0]}
                        contract.run(_krylov_fn(driver, reortho, op, params, V, k, contract, tally), what, repeats=3)
                        print(f"{what}: graph captures / replays {tally}")
                        for direction, (captured, replayed) in tally.items():
                            captures["lanczos" if (driver, reortho) == ("lanczos", "none") else "arnoldi", direction] += captured
                            assert not graphs or replayed >= 1, (what, direction, captured, replayed)
    assert not graphs or all(count >= 1 for count in captures.values()), captures


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("opkind", ["gram", "dense"])
def test_krylov_drivers_eager_captured_and_replayed(contract, opkind, dtype):
    _krylov_sweep(contract, opkind, dtype)


def _probe_group_child():
    _krylov_sweep(Contract(_installed), "gram", F32, ks=(7,), ps=(5,))
    print("child ok")


def test_adjoints_with_forced_probe_groups():
    """MFX_PROBE_GROUP is read once per process: groups of 2, 2 and 1 probes in a child process"""
    root = os.path.dirname(HERE)
    code = (f"import sys\nfor q in ({HERE!r}, {root!r}, {os.path.join(root, 'experiments-lanczos-adjoints_amd')!r}):\n    sys.path.insert(0, q)\n"
            "import test_gpu_workspace_contract as t\nt._probe_group_child()\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, MFX_PROBE_GROUP="2"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("cdtype", [torch.complex64, torch.complex128], ids=["c64", "c128"])
def test_complex_arnoldi_forward(contract, cdtype):
    n, k, p = 64, 5, 2
    rdt = F32 if cdtype == torch.complex64 else F64
    A = torch.complex(randn((n, n), rdt, 21), randn((n, n), rdt, 22)) / math.sqrt(n)
    V = torch.complex(randn((p, n), rdt, 23), randn((p, n), rdt, 24))

    def fn():
        with torch.no_grad():
            return named("out", [t.contiguous() for t in arnoldi.hessenberg(DenseOp(), k, reortho="full")(V, A)])

    contract.run(fn, "mfx_arnoldi_forward_complex")


def test_callback_operator_reenters_the_allocator(contract):
    """a Python matvec that calls the native Gram operator: the inner call asks for a workspace while the outer driver holds its own"""
    n, k, p = 300, 7, 3
    op, params = gram(n, 3, F64)
    V = randn((p, n), F64, 31)
    nested = []  # per guarded matvec: (workspaces in use when it starts, workspaces the guarded allocator handed out during it)

    def matvec(v, *q):
        busy, before = set(_lib._ws_busy), contract.guard.handed_out
        y = op(v, *q)
        if contract.guarded:
            nested.append((busy, contract.guard.handed_out - before))
        return y

    cb = CallbackOp(matvec)

    def fn():
        (basis, (diag, off)), (q, b) = lanczos.tridiag(cb, k, reortho="full")(V, *params)
        outs = (basis, diag, off, q, b)
        return {**named("out", outs), **named("g", grads_of(outs, params))}

    contract.run(fn, "callback operator around a native one")
    # the re-entry happened: every nested application took a workspace of its own while the driver's was marked busy, and that
    # workspace is another buffer than the driver's
    assert len(nested) >= 2 * k * p
    outer = {i for busy, _ in nested for i in busy}
    views = {id(rec.view): rec for recs in contract.guard._pool.values() for rec in recs}
    assert all(len(busy) == 1 and taken >= 1 for busy, taken in nested), nested[:3]
    assert outer <= set(views) and len(views) > len(outer)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_slq_value_and_gradient(contract, dtype):
    """integrand_spd: the deferred parameter sweep batches p (k + 1) rows"""
    n, k, p = 300, 7, 5
    op, params = gram(n, 8, dtype)
    V = torch.sign(randn((p, n), dtype, 41))
    integrand = lanczos.integrand_spd(torch.log, k, op)

    def fn():
        val = integrand(V, *params)
        return {"value": val, **named("g", torch.autograd.grad(val.sum(), params))}

    contract.run(fn, "SLQ integrand_spd")


def test_eigh_and_quadform_leading_dimensions():
    """ldbeta of mfx_tridiag_eigh (an input) and lddbeta of mfx_slq_quadform_bwd (an output): the padding plays no part and survives"""
    lib = _lib.get()
    p, k, ld = 5, 7, 9
    for dtype in (F32, F64):
        code = _lib.dtype_code(dtype)
        alpha = 2.0 + randn((p, k), dtype, 51).abs()
        beta = 0.2 * randn((p, k - 1), dtype, 52)  # (diagonally dominant: positive eigenvalues for the logarithm below)
        res = []
        for pad in (None, SENT, float("nan")):
            b = beta.clone() if pad is None else torch.full((p, ld), pad, dtype=dtype, device=DEV)
            if pad is not None:
                b[:, : k - 1] = beta
            evals, evecs = torch.empty((p, k), dtype=dtype, device=DEV), torch.empty((p, k, k), dtype=dtype, device=DEV)
            _lib.check(lib.mfx_tridiag_eigh(_lib.ptr(alpha), _lib.ptr(b), b.stride(0), p, k, code, _lib.ptr(evals), _lib.ptr(evecs),
                                            _lib.stream_ptr(DEV)))
            torch.cuda.synchronize()
            if pad is not None:
                tail = b[:, k - 1 :]
                assert bool((tail == pad).all() if pad == pad else torch.isnan(tail).all()) and torch.equal(b[:, : k - 1], beta)
            res.append((evals, evecs))
        for evals, evecs in res[1:]:
            assert torch.equal(evals, res[0][0]) and torch.equal(evecs, res[0][1])
        evals, evecs = res[0]
        assert bool(torch.isfinite(evals).all())
        fx, dfx, gout = torch.log(evals), 1.0 / evals, randn((p,), dtype, 53)
        outs = []
        for width in (k - 1, ld):
            dalpha = torch.empty((p, k), dtype=dtype, device=DEV)
            dbeta = torch.full((p, width), SENT, dtype=dtype, device=DEV)
            _lib.check(lib.mfx_slq_quadform_bwd(_lib.ptr(evals), _lib.ptr(evecs), _lib.ptr(fx), _lib.ptr(dfx), _lib.ptr(gout), p, k, code,
                                                _lib.ptr(dalpha), _lib.ptr(dbeta), width, _lib.stream_ptr(DEV)))
            torch.cuda.synchronize()
            assert bool((dbeta[:, k - 1 :] == SENT).all()), "mfx_slq_quadform_bwd wrote into the padding of dbeta"
            outs.append((dalpha, dbeta[:, : k - 1]))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert bool(torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all())


# ---------------------------------------------------------------------------------------------------------------------------
# solvers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 5])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_solvers(contract, dtype, p):
    n, rank = 300, 8
    op, params = gram(n, 8, dtype)
    bound = op.bind(*params)
    B = randn((p, n), dtype, 61).requires_grad_(True)
    shift = float(op.constrain(*params)[2].detach())

    chols = {}
    for pivot in (False, True):
        make = (low_rank.cholesky_partial_pivot if pivot else low_rank.cholesky_partial)(rank=rank)

        def fn(make=make):
            chol, _info = make(bound, n)
            return {"chol": chol.contiguous()}

        chols[pivot] = contract.run(fn, f"mfx_partial_cholesky pivot={pivot}")["chol"]
    pre = low_rank.Preconditioner(chols[True].to(DEV))
    P = pre.bind(shift)

    contract.run(lambda: {"z": pre(B.detach(), shift)}, "mfx_precond_apply")
    contract.run(lambda: {"z": pre.sample(3, p, shift)}, "mfx_precond_sample", uses_ws=False)

    def solve_fn(solver, precond, extras=()):
        def fn():
            x, info = solver(bound, B, precond)
            out = {"x": x, "r": info["residual_abs"], **named("g", grads_of((x,), (B, *params)))}
            for key in extras:
                val = info[key]
                out.update(named(key, val) if isinstance(val, tuple) else {key: val})
            return out

        return fn

    for precond in (None, P):
        tag = "preconditioned" if precond is not None else "plain"
        contract.run(solve_fn(cg.pcg_fixed_step(10), precond), f"mfx_pcg_solve fixed {tag}")
        contract.run(solve_fn(cg.pcg_adaptive(atol=1e-3, rtol=1e-3, maxiter=25, miniter=2), precond, ("num_steps",)),
                     f"mfx_pcg_solve adaptive {tag}")
        contract.run(solve_fn(cg.pcg_fixed_step_reortho(6), precond, ("Q",)), f"mfx_pcg_solve_reortho {tag}")
        contract.run(solve_fn(cg.mbcg_fixed_step(20), precond, ("num_steps", "tridiag", "rz0", "depth", "w0")), f"mfx_mbcg_solve {tag}")


# ---------------------------------------------------------------------------------------------------------------------------
# cross-covariance family (ctypes: the request subsets decide which sweeps launch)
# ---------------------------------------------------------------------------------------------------------------------------
SUBSETS = [("theta",), ("xnew",), ("x",), ("theta", "x"), ("theta", "xnew", "x")]


def _cross_problem(n, d, m, dtype, ard):
    op, params = gram(n, d, dtype, ard=ard)
    cparams = [q.detach() for q in op.constrain(*params)]
    return op, cparams, randn((m, d), dtype, 71 + m)


def _cross_grads(cparams, xnew, X, subset):
    st, out = _lib.OpGrads(), {}
    if "theta" in subset:
        out["gls"], out["gs"] = torch.zeros_like(cparams[0]), torch.zeros_like(cparams[1])
        st.lengthscale, st.outputscale = out["gls"].data_ptr(), out["gs"].data_ptr()
    if "x" in subset:
        out["gx"] = torch.zeros_like(X)
        st.x = out["gx"].data_ptr()
    if "xnew" in subset:
        out["gxnew"] = torch.zeros_like(xnew)
    return st, out


@pytest.mark.parametrize("n", [300, 2049])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_cross_covariance_family(contract, dtype, n):
    lib, stream, p = _lib.get(), _lib.stream_ptr(DEV), 3
    for d in (3, 20, 40):
        for ard in (True, False):
            for m in (1, 70):
                op, cparams, xnew = _cross_problem(n, d, m, dtype, ard)
                what = f"d={d} ard={ard} m={m} n={n}"
                v, u = randn((p, n), dtype, 81), randn((p, m), dtype, 82)

                def apply_fn(transposed):
                    def fn():
                        desc = op.descriptor(cparams, dtype, n)
                        ws = _lib.scratch(int(lib.mfx_gram_cross_workspace_bytes(C.byref(desc), m)), DEV)
                        width = n if transposed else m
                        y = torch.full((p, width + 5), SENT, dtype=dtype, device=DEV)
                        call = lib.mfx_gram_cross_apply_t if transposed else lib.mfx_gram_cross_apply
                        src = u if transposed else v
                        _lib.check(call(C.byref(desc), _lib.ptr(xnew), m, _lib.ptr(src), src.stride(0), _lib.ptr(y), width + 5, p,
                                        _lib.ptr(ws), ws.numel(), stream))
                        assert bool((y[:, width:] == SENT).all()), "the padding of y was written"
                        return {"y": y[:, :width]}

                    return fn

                contract.run(apply_fn(False), f"mfx_gram_cross_apply {what}")
                contract.run(apply_fn(True), f"mfx_gram_cross_apply_t {what}")

                for batch in (1, 33):
                    L, R = randn((batch, m), dtype, 83), randn((batch, n), dtype, 84)
                    for subset in SUBSETS:
                        def fn(batch=batch, L=L, R=R, subset=subset):
                            desc = op.descriptor(cparams, dtype, n)
                            st, out = _cross_grads(cparams, xnew, op.X, subset)
                            ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_workspace_bytes(C.byref(desc), m, batch)), DEV)
                            _lib.check(lib.mfx_gram_cross_vjp(C.byref(desc), _lib.ptr(xnew), m, _lib.ptr(L), m, _lib.ptr(R), n, batch,
                                                              C.byref(st), _lib.ptr(out.get("gxnew")), _lib.ptr(ws), ws.numel(), stream))
                            return out

                        contract.run(fn, f"mfx_gram_cross_vjp {what} batch={batch} {'+'.join(subset)}")

                for lds in ((n + 3) // 4 * 4, (n + 3) // 4 * 4 + 1):  # 16-byte aligned rows (vector loads) and odd
                    S = randn((m, lds), dtype, 85)
                    for subset in SUBSETS:
                        def fn(S=S, lds=lds, subset=subset):
                            desc = op.descriptor(cparams, dtype, n)
                            st, out = _cross_grads(cparams, xnew, op.X, subset)
                            ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_dense_workspace_bytes(C.byref(desc), m)), DEV)
                            _lib.check(lib.mfx_gram_cross_vjp_dense(C.byref(desc), _lib.ptr(xnew), m, _lib.ptr(S), lds, C.byref(st),
                                                                    _lib.ptr(out.get("gxnew")), _lib.ptr(ws), ws.numel(), stream))
                            return out

                        contract.run(fn, f"mfx_gram_cross_vjp_dense {what} lds={lds} {'+'.join(subset)}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_gram_block_with_padded_output(contract, dtype):
    lib, stream = _lib.get(), _lib.stream_ptr(DEV)
    for d in (3, 20, 40):
        for ard in (True, False):
            for ma, mb in ((1, 70), (70, 65)):
                op, cparams, xa = _cross_problem(mb, d, ma, dtype, ard)
                xb, ldo = op.X, mb + 3

                def fn():
                    desc = op.descriptor(cparams, dtype, mb)
                    ws = _lib.scratch(int(lib.mfx_gram_block_workspace_bytes(C.byref(desc), ma, mb)), DEV)
                    out = torch.full((ma, ldo), SENT, dtype=dtype, device=DEV)
                    _lib.check(lib.mfx_gram_block(C.byref(desc), _lib.ptr(xa), ma, _lib.ptr(xb), mb, _lib.ptr(out), ldo, _lib.ptr(ws),
                                                  ws.numel(), stream))
                    assert bool((out[:, mb:] == SENT).all()), "mfx_gram_block wrote into the padding of out"
                    return {"K": out[:, :mb]}

                contract.run(fn, f"mfx_gram_block d={d} ard={ard} ({ma}, {mb})")


# ---------------------------------------------------------------------------------------------------------------------------
# row-sharded drivers: two logical ranks as threads (the stage / send / gathered / xfull regions)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_row_sharded_drivers(contract, dtype):
    from _local_world import LocalWorld
    from matfree_extensions.distributed import RowComm

    n, k, p = 256, 5, 3
    op, params = gram(n, 8, dtype)
    V, B = randn((p, n), dtype, 91), randn((p, n), dtype, 92)
    V = V / V.norm(dim=-1, keepdim=True)

    def body(handle):
        comm = RowComm(n, group=handle)
        sop = RowShardedOp(op, comm)
        mine = [q.detach().clone().requires_grad_(True) for q in params]
        Vl = comm.rows(V).requires_grad_(True)
        out = {}
        (basis, (diag, off)), (q, b) = lanczos.tridiag(sop, k, reortho="none")(Vl, *mine)
        outs = (basis, diag, off, q, b)
        out.update(named("lanczos", outs), **named("lanczos_g", grads_of(outs, (Vl, *mine))))
        outs = arnoldi.hessenberg(sop, k, reortho="full")(Vl, *mine)
        out.update(named("arnoldi", outs), **named("arnoldi_g", grads_of(outs, (Vl, *mine))))
        x, info = cg.pcg_fixed_step(8)(sop.bind(*mine), comm.rows(B), None)
        out.update(pcg_x=x, pcg_r=info["residual_abs"])
        return _cpu(out)

    def fn():
        return {f"rank{r}_{key}": t for r, res in enumerate(LocalWorld(2).run(body)) for key, t in res.items()}

    contract.run(fn, "row-sharded drivers on two logical ranks")


# ---------------------------------------------------------------------------------------------------------------------------
# exact size accepted, 255 bytes refused before any launch: once per workspace-taking entry point, through ctypes
# ---------------------------------------------------------------------------------------------------------------------------
class _Small:
    """the shared inputs of the entry-point builders below: (n, d, p) = (300, 3, 1) in fp32, the smallest row of the tables"""

    n, d, p, k, m, rank, dt = 300, 3, 1, 2, 1, 8, F32

    def __init__(self):
        self.lib, self.stream = _lib.get(), _lib.stream_ptr(DEV)
        self.op, self.params = gram(self.n, self.d, self.dt)
        self.cparams = [q.detach() for q in self.op.constrain(*self.params)]
        self.desc = self.op.descriptor(self.cparams, self.dt, self.n)
        self.od = C.byref(self.desc)
        V = randn((self.p, self.n), self.dt, 101)
        self.V = V / V.norm(dim=-1, keepdim=True)
        self.W = randn((self.p, self.n), self.dt, 102)
        self.xnew, self.u = randn((self.m, self.d), self.dt, 109), randn((self.p, self.m), self.dt, 110)
        self.need_k = int(self.lib.mfx_workspace_bytes(self.od, self.n, self.k, self.p))
        self.need_1 = int(self.lib.mfx_workspace_bytes(self.od, self.n, 1, self.p))

    def new(self, *shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.dt, device=DEV)

    def grads(self, noise=True, x=False):
        """-> (mfx_op_grads, the tensors it points to)"""
        g = [self.new(self.cparams[0].numel()), self.new(1)] + ([self.new(1)] if noise else []) + ([self.new(self.n, self.d)] if x else [])
        st = _lib.OpGrads()
        st.lengthscale, st.outputscale = g[0].data_ptr(), g[1].data_ptr()
        if noise:
            st.noise = g[2].data_ptr()
        if x:
            st.x = g[-1].data_ptr()
        return st, g


# each builder -> (need, outputs, call(ws, ws_bytes) -> rc); what a closure uses stays alive through the closure
def _ep_op_apply(s):
    y = s.new(s.p, s.n)
    return s.need_1, [y], lambda ws, nb: s.lib.mfx_op_apply(s.od, _lib.ptr(s.V), s.n, _lib.ptr(y), s.n, s.p, 0, _lib.ptr(ws), nb, s.stream)


def _ep_op_vjp_params(s):
    st, g = s.grads()
    return s.need_1, g, lambda ws, nb: s.lib.mfx_op_vjp_params(s.od, _lib.ptr(s.W), s.n, _lib.ptr(s.V), s.n, s.p, C.byref(st),
                                                              _lib.ptr(ws), nb, s.stream)


def _ep_arnoldi_forward(s):
    Q, H, r, c = s.new(s.p, s.k, s.n), s.new(s.p, s.k, s.k), s.new(s.p, s.n), s.new(s.p)
    return s.need_k, [Q, H, r, c], lambda ws, nb: s.lib.mfx_arnoldi_forward(
        s.od, _lib.ptr(s.V), s.n, s.k, s.p, 1, _lib.ptr(Q), _lib.ptr(H), _lib.ptr(r), _lib.ptr(c), _lib.ptr(ws), nb, s.stream)


def _ep_arnoldi_adjoint(s):
    with torch.no_grad():  # a forward result, made with an ordinary workspace
        Q, H, r, c = arnoldi.hessenberg(s.op, s.k, reortho="full")(s.V, *s.params)
    Q, H, r, c = Q.transpose(-1, -2).contiguous(), H.contiguous(), r.contiguous(), c.contiguous()  # Q: storage (p, k, n)
    dH = randn((s.p, s.k, s.k), s.dt, 103)
    dv, Lam = s.new(s.p, s.n), s.new(s.p, s.k, s.n)
    st, g = s.grads()
    return s.need_k, [dv, Lam, *g], lambda ws, nb: s.lib.mfx_arnoldi_adjoint(
        s.od, s.n, s.k, s.p, _lib.ptr(Q), _lib.ptr(H), _lib.ptr(r), _lib.ptr(c), None, _lib.ptr(dH), None, None, _lib.REORTHO_FULL,
        _lib.ptr(dv), _lib.ptr(Lam), C.byref(st), _lib.ptr(ws), nb, s.stream)


def _ep_lanczos_forward(s):
    xs, alpha, beta, vnorm = s.new(s.p, s.k + 1, s.n), s.new(s.p, s.k), s.new(s.p, s.k), s.new(s.p)
    return s.need_k, [xs, alpha, beta, vnorm], lambda ws, nb: s.lib.mfx_lanczos_forward(
        s.od, _lib.ptr(s.V), s.n, s.k, s.p, _lib.ptr(xs), _lib.ptr(alpha), _lib.ptr(beta), _lib.ptr(vnorm), _lib.ptr(ws), nb, s.stream)


def _ep_lanczos_adjoint(s):
    with torch.no_grad():
        xs, alpha, beta = (t.contiguous() for t in lanczos._LanczosFn.apply(s.op, s.k, True, s.V, *s.cparams))
    vnorm = torch.linalg.vector_norm(s.V, dim=-1)
    dal, dbe = randn((s.p, s.k), s.dt, 104), randn((s.p, s.k), s.dt, 105)
    dv, Lam = s.new(s.p, s.n), s.new(s.p, s.k, s.n)
    st, g = s.grads()
    return s.need_k, [dv, Lam, *g], lambda ws, nb: s.lib.mfx_lanczos_adjoint(
        s.od, s.n, s.k, s.p, _lib.ptr(xs), _lib.ptr(alpha), _lib.ptr(beta), _lib.ptr(vnorm), None, _lib.ptr(dal), _lib.ptr(dbe),
        _lib.ptr(dv), _lib.ptr(Lam), C.byref(st), _lib.ptr(ws), nb, s.stream)


def _ep_arnoldi_forward_complex(s):
    n, k, p = 64, 5, 2  # interleaved (re, im) reals; the operator is the (2 n, 2 n) real form
    M = randn((2 * n, 2 * n), s.dt, 106) / math.sqrt(n)
    desc = DenseOp().descriptor((M,), s.dt, 2 * n)
    v0 = randn((p, n, 2), s.dt, 107)
    Q, H, r, c = s.new(p, k, n, 2), s.new(p, k, k, 2), s.new(p, n, 2), s.new(p, 2)
    need = int(s.lib.mfx_complex_workspace_bytes(C.byref(desc), n, k, p))
    return need, [Q, H, r, c], lambda ws, nb, _matrix=M: s.lib.mfx_arnoldi_forward_complex(  # (_matrix: desc only borrows its pointer)
        C.byref(desc), _lib.ptr(v0), n, k, p, 1, _lib.ptr(Q), _lib.ptr(H), _lib.ptr(r), _lib.ptr(c), _lib.ptr(ws), nb, s.stream)


def _ep_pcg_solve(s):
    x, r, steps = s.new(s.p, s.n), s.new(s.p, s.n), s.new(s.p, dtype=torch.int64)
    need = int(s.lib.mfx_pcg_workspace_bytes(s.od, s.n, s.p, 0))
    return need, [x, r, steps], lambda ws, nb: s.lib.mfx_pcg_solve(
        s.od, _lib.ptr(s.W), s.n, s.n, s.p, None, 0, None, None, 5, 0, 1.0, 0.0, 0, _lib.ptr(x), _lib.ptr(r), _lib.ptr(steps), _lib.ptr(ws), nb,
        s.stream)


def _ep_pcg_solve_reortho(s):
    x, r, q = s.new(s.p, s.n), s.new(s.p, s.n), s.new(s.p, 4, s.n)
    need = int(s.lib.mfx_pcg_workspace_bytes(s.od, s.n, s.p, 4))
    return need, [x, r, q], lambda ws, nb: s.lib.mfx_pcg_solve_reortho(
        s.od, _lib.ptr(s.W), s.n, s.n, s.p, None, 0, None, None, 4, _lib.ptr(x), _lib.ptr(r), _lib.ptr(q), _lib.ptr(ws), nb, s.stream)


def _ep_precond_apply(s):
    lt = 0.1 * randn((s.rank, s.n), s.dt, 108)
    minv = torch.linalg.inv((lt @ lt.T).double() + torch.eye(s.rank, dtype=F64, device=DEV)).to(s.dt).contiguous()
    shift = torch.ones(1, dtype=s.dt, device=DEV)
    z = s.new(s.p, s.n)
    need = int(s.lib.mfx_pcg_workspace_bytes(s.od, s.n, s.p, s.rank))
    return need, [z], lambda ws, nb: s.lib.mfx_precond_apply(
        _lib.MFX_F32, s.n, s.rank, _lib.ptr(lt), _lib.ptr(minv), _lib.ptr(shift), _lib.ptr(s.W), s.n, _lib.ptr(z), s.n, s.p, _lib.ptr(ws), nb,
        s.stream)


def _ep_mbcg_solve(s):
    mi = 20
    x, r, steps, w0 = s.new(s.p, s.n), s.new(s.p, s.n), s.new(s.p, dtype=torch.int64), s.new(s.p, s.n)
    td, to, rz0, depth = s.new(s.p, mi), s.new(s.p, mi), s.new(s.p), s.new(s.p, dtype=torch.int64)
    need = int(s.lib.mfx_mbcg_workspace_bytes(s.od, s.n, s.p, 0, mi))
    return need, [x, r, steps, w0, td, to, rz0, depth], lambda ws, nb: s.lib.mfx_mbcg_solve(
        s.od, _lib.ptr(s.W), s.n, s.n, s.p, None, 0, None, None, mi, 0, 1.0, 0.0, 0, _lib.ptr(x), _lib.ptr(r), _lib.ptr(steps), _lib.ptr(w0),
        _lib.ptr(td), _lib.ptr(to), _lib.ptr(rz0), _lib.ptr(depth), _lib.ptr(ws), nb, s.stream)


def _ep_partial_cholesky(s):
    lt, piv, ok = s.new(s.rank, s.n), s.new(s.rank, dtype=torch.int64), s.new(1, dtype=torch.int32)
    need = int(s.lib.mfx_pcg_workspace_bytes(s.od, s.n, 1, s.rank))
    return need, [lt, piv, ok], lambda ws, nb: s.lib.mfx_partial_cholesky(
        s.od, s.rank, 1, 1, _lib.ptr(lt), _lib.ptr(piv), _lib.ptr(ok), _lib.ptr(ws), nb, s.stream)


def _ep_gram_cross_apply(s):
    y = s.new(s.p, s.m)
    need = int(s.lib.mfx_gram_cross_workspace_bytes(s.od, s.m))
    return need, [y], lambda ws, nb: s.lib.mfx_gram_cross_apply(
        s.od, _lib.ptr(s.xnew), s.m, _lib.ptr(s.V), s.n, _lib.ptr(y), s.m, s.p, _lib.ptr(ws), nb, s.stream)


def _ep_gram_cross_apply_t(s):
    y = s.new(s.p, s.n)
    need = int(s.lib.mfx_gram_cross_workspace_bytes(s.od, s.m))
    return need, [y], lambda ws, nb: s.lib.mfx_gram_cross_apply_t(
        s.od, _lib.ptr(s.xnew), s.m, _lib.ptr(s.u), s.m, _lib.ptr(y), s.n, s.p, _lib.ptr(ws), nb, s.stream)


def _ep_gram_cross_vjp(s):
    st, g = s.grads(noise=False, x=True)
    gxnew = s.new(s.m, s.d)
    need = int(s.lib.mfx_gram_cross_vjp_workspace_bytes(s.od, s.m, s.p))
    return need, [*g, gxnew], lambda ws, nb: s.lib.mfx_gram_cross_vjp(
        s.od, _lib.ptr(s.xnew), s.m, _lib.ptr(s.u), s.m, _lib.ptr(s.V), s.n, s.p, C.byref(st), _lib.ptr(gxnew), _lib.ptr(ws), nb, s.stream)


def _ep_gram_cross_vjp_dense(s):
    st, g = s.grads(noise=False, x=True)
    gxnew, S = s.new(s.m, s.d), randn((s.m, s.n), s.dt, 111)
    need = int(s.lib.mfx_gram_cross_vjp_dense_workspace_bytes(s.od, s.m))
    return need, [*g, gxnew], lambda ws, nb: s.lib.mfx_gram_cross_vjp_dense(
        s.od, _lib.ptr(s.xnew), s.m, _lib.ptr(S), s.n, C.byref(st), _lib.ptr(gxnew), _lib.ptr(ws), nb, s.stream)


def _ep_gram_block(s):
    xb, K = randn((70, s.d), s.dt, 112), s.new(s.m, 70)
    need = int(s.lib.mfx_gram_block_workspace_bytes(s.od, s.m, 70))
    return need, [K], lambda ws, nb: s.lib.mfx_gram_block(
        s.od, _lib.ptr(s.xnew), s.m, _lib.ptr(xb), 70, _lib.ptr(K), 70, _lib.ptr(ws), nb, s.stream)


ENTRY_POINTS = {
    "mfx_op_apply": _ep_op_apply, "mfx_op_vjp_params": _ep_op_vjp_params, "mfx_arnoldi_forward": _ep_arnoldi_forward,
    "mfx_arnoldi_adjoint": _ep_arnoldi_adjoint, "mfx_lanczos_forward": _ep_lanczos_forward, "mfx_lanczos_adjoint": _ep_lanczos_adjoint,
    "mfx_arnoldi_forward_complex": _ep_arnoldi_forward_complex, "mfx_pcg_solve": _ep_pcg_solve,
    "mfx_pcg_solve_reortho": _ep_pcg_solve_reortho, "mfx_precond_apply": _ep_precond_apply, "mfx_mbcg_solve": _ep_mbcg_solve,
    "mfx_partial_cholesky": _ep_partial_cholesky, "mfx_gram_cross_apply": _ep_gram_cross_apply,
    "mfx_gram_cross_apply_t": _ep_gram_cross_apply_t, "mfx_gram_cross_vjp": _ep_gram_cross_vjp,
    "mfx_gram_cross_vjp_dense": _ep_gram_cross_vjp_dense, "mfx_gram_block": _ep_gram_block,
}


def _refused_then_accepted(guard, name, need, outs, call):
    """255 bytes: MFX_ERR_WORKSPACE with outputs, workspace and guards untouched; the queried size: accepted, guards untouched"""
    assert need > 255, (name, need)
    ws = guard.take(need, DEV, label=name)
    assert ws.numel() == need and ws.data_ptr() % 256 == 0
    for t in outs:
        t.fill_(SENT)
    rc = call(ws, 255)
    torch.cuda.synchronize()
    assert rc == MFX_ERR_WORKSPACE, f"{name}: 255 bytes of workspace gave {rc}, not MFX_ERR_WORKSPACE"
    for i, t in enumerate(outs):
        assert bool((t == SENT).all()), f"{name}: output {i} was written although the call was refused"
    assert bool((ws == guard.poison).all()), f"{name}: the workspace was written although the call was refused"
    guard.verify()
    rc = call(ws, need)
    torch.cuda.synchronize()
    assert rc == 0, f"{name}: refused its own queried size {need}: {_lib.get().mfx_last_error().decode()}"
    guard.verify()


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_exact_size_is_accepted_and_a_short_workspace_is_refused_before_any_launch(name):
    small = _Small()
    need, outs, call = ENTRY_POINTS[name](small)
    for poison in (0x00, 0xFF):
        _refused_then_accepted(GuardedWs(poison), name, need, outs, call)


def test_sharded_entry_points_refuse_a_short_workspace_on_every_rank_before_any_collective():
    """The five row-sharded entry points on two logical ranks: a refusal that came after the first collective of one rank would
    strand the other, so rc == MFX_ERR_WORKSPACE on BOTH ranks with outputs, workspace and guards untouched, then the queried size
    is accepted.  The adjoints take what the accepted forward call of the same rank wrote."""
    from _local_world import LocalWorld
    from matfree_extensions.distributed import RowComm

    lib, dt = _lib.get(), F32
    n, k, p = 256, 2, 1
    op, params = gram(n, 3, dt)
    cparams = [q.detach() for q in op.constrain(*params)]
    V, B = randn((p, n), dt, 121), randn((p, n), dt, 122)
    V = V / V.norm(dim=-1, keepdim=True)
    guards = {0x00: GuardedWs(0x00), 0xFF: GuardedWs(0xFF)}

    def body(handle):
        comm = RowComm(n, group=handle)
        nr, stream = comm.nrows, _lib.stream_ptr(DEV)
        desc = op.descriptor(cparams, dt, n)
        od = C.byref(desc)
        cm0 = _lib.Comm()
        cm0.rank, cm0.world, cm0.nloc = comm.rank, comm.world, comm.nloc
        need_k = int(lib.mfx_sharded_workspace_bytes(od, C.byref(cm0), n, k, p))
        need_cg = int(lib.mfx_pcg_sharded_workspace_bytes(od, C.byref(cm0), n, p, 0))

        def new(*shape, dtype=dt):
            return torch.empty(shape, dtype=dtype, device=DEV)

        def grads():
            g = [new(cparams[0].numel()), new(1), new(1)]
            st = _lib.OpGrads()
            st.lengthscale, st.outputscale, st.noise = (t.data_ptr() for t in g)
            return st, g

        Vl, Bl = comm.rows(V), comm.rows(B)
        xs, alpha, beta, vnorm = new(p, k + 1, nr), new(p, k), new(p, k), new(p)
        Q, Qfull, H, r, c = new(p, k, nr), new(p, k, n), new(p, k, k), new(p, nr), new(p)
        dal, dbe, dH = randn((p, k), dt, 123), randn((p, k), dt, 124), randn((p, k, k), dt, 125)
        dv1, Lam1, Lamfull = new(p, nr), new(p, k, nr), new(p, k, n)
        dv2, Lam2 = new(p, nr), new(p, k, nr)
        st1, g1 = grads()
        st2, g2 = grads()
        x, res, steps = new(p, nr), new(p, nr), new(p, dtype=torch.int64)
        # (name, need, outputs, tensors the collective callbacks may be handed besides the workspace, call(comm struct, ws, ws_bytes))
        entries = [
            ("mfx_lanczos_forward_sharded", need_k, [xs, alpha, beta, vnorm], (xs,), lambda cm, ws, nb: lib.mfx_lanczos_forward_sharded(
                od, C.byref(cm), _lib.ptr(Vl), n, k, p, _lib.ptr(xs), _lib.ptr(alpha), _lib.ptr(beta), _lib.ptr(vnorm), _lib.ptr(ws), nb, stream)),
            ("mfx_lanczos_adjoint_sharded", need_k, [dv1, Lam1, Lamfull, *g1], (Lam1, Lamfull),
             lambda cm, ws, nb: lib.mfx_lanczos_adjoint_sharded(
                 od, C.byref(cm), n, k, p, _lib.ptr(xs), _lib.ptr(alpha), _lib.ptr(beta), _lib.ptr(vnorm), None, _lib.ptr(dal), _lib.ptr(dbe),
                 _lib.ptr(dv1), _lib.ptr(Lam1), _lib.ptr(Lamfull), C.byref(st1), _lib.ptr(ws), nb, stream)),
            ("mfx_arnoldi_forward_sharded", need_k, [Q, Qfull, H, r, c], (Q, Qfull), lambda cm, ws, nb: lib.mfx_arnoldi_forward_sharded(
                od, C.byref(cm), _lib.ptr(Vl), n, k, p, 1, _lib.ptr(Q), _lib.ptr(Qfull), _lib.ptr(H), _lib.ptr(r), _lib.ptr(c), _lib.ptr(ws), nb,
                stream)),
            ("mfx_arnoldi_adjoint_sharded", need_k, [dv2, Lam2, *g2], (Lam2,), lambda cm, ws, nb: lib.mfx_arnoldi_adjoint_sharded(
                od, C.byref(cm), n, k, p, _lib.ptr(Q), _lib.ptr(Qfull), _lib.ptr(H), _lib.ptr(r), _lib.ptr(c), None, _lib.ptr(dH), None, None,
                _lib.REORTHO_FULL, _lib.ptr(dv2), _lib.ptr(Lam2), C.byref(st2), _lib.ptr(ws), nb, stream)),
            ("mfx_pcg_solve_sharded", need_cg, [x, res, steps], (), lambda cm, ws, nb: lib.mfx_pcg_solve_sharded(
                od, C.byref(cm), _lib.ptr(Bl), nr, n, p, None, 0, None, None, 5, 0, 1.0, 0.0, 0, _lib.ptr(x), _lib.ptr(res), _lib.ptr(steps),
                _lib.ptr(ws), nb, stream)),
        ]
        codes = []
        for poison, guard in guards.items():
            for name, need, outs, extra, call in entries:
                assert need > 255, (name, need)
                ws = guard.take(need, DEV, label=f"{name} rank {comm.rank}")
                keep_inputs = [t.clone() for t in outs]  # (the forward outputs are the adjoints' inputs: put back after the refusal)
                for t in outs:
                    t.fill_(SENT)
                cm, keep = comm.struct(ws, tensors=extra)
                with _lib.busy(ws):
                    rc = call(cm, ws, 255)
                torch.cuda.synchronize()
                codes.append((name, poison, "short", rc))
                clean = all(bool((t == SENT).all()) for t in outs) and bool((ws == poison).all())
                codes.append((name, poison, "untouched", clean))
                for t, old in zip(outs, keep_inputs):
                    t.copy_(old)
                if rc != MFX_ERR_WORKSPACE:  # (every rank takes this branch or none does, unless the refusal itself is broken;
                    break                    #  a rank left alone in a collective is released by the world's barrier timeout)
                with _lib.busy(ws):
                    rc = call(cm, ws, need)
                torch.cuda.synchronize()
                assert not keep[2], keep[2]
                codes.append((name, poison, "exact", rc))
        return codes

    results = LocalWorld(2, timeout=30.0).run(body)
    for guard in guards.values():
        guard.verify()
    assert results[0] == results[1]
    for rank, codes in enumerate(results):
        for name, poison, what, value in codes:
            want = {"short": MFX_ERR_WORKSPACE, "untouched": True, "exact": 0}[what]
            assert value == want, f"rank {rank}: {name} (poison 0x{poison:02X}) {what}: {value}"
        assert len(codes) == 2 * 5 * 3


def test_partial_cholesky_refuses_rank_zero_before_any_launch():
    lib = _lib.get()
    n = 300
    op, params = gram(n, 3, F32)
    cparams = [q.detach() for q in op.constrain(*params)]
    desc = op.descriptor(cparams, F32, n)
    guard = GuardedWs(0xFF)
    need = int(lib.mfx_pcg_workspace_bytes(C.byref(desc), n, 1, 0))
    ws = guard.take(need, DEV, label="mfx_partial_cholesky rank 0")
    lt = torch.full((1, n), SENT, device=DEV)
    piv = torch.full((1,), -77, dtype=torch.int64, device=DEV)
    ok = torch.full((1,), -77, dtype=torch.int32, device=DEV)
    rc = lib.mfx_partial_cholesky(C.byref(desc), 0, 1, 1, _lib.ptr(lt), _lib.ptr(piv), _lib.ptr(ok), _lib.ptr(ws), need, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == MFX_ERR_INVALID
    assert bool((lt == SENT).all()) and int(piv) == -77 and int(ok) == -77 and bool((ws == 0xFF).all())
    guard.verify()
