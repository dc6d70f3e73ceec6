"""The matrix-free GGN operator of an MLP on the GPU against the NumPy restatement (tests/_ggn_restatement.py).

Geometry of the shipped kernels (csrc/mfx_ggn.hip): a workgroup takes tiles of 32 samples and a group of 4 (fp32) / 2 (fp64) probes;
layers past the input are one chunk of at most 64 units, the input is streamed in chunks of 64 columns; at most 64 workgroups along
the samples, so N > 2048 makes a workgroup walk more than one tile.  Shapes: N in {1, 63, 64, 65, 257} (and 2081 for the tile loop),
widths with L = 1, a 64-wide layer, d_in = 130 (three chunks, the last ragged), one-unit layers and c = 1; p in {1, 3, 5}.

Bound of the apply.  The restatement is fed the operator's own tape, upcast exactly, so only the kernel's arithmetic is judged:
|y - y_ref| <= gamma eps s entrywise with s = |A| |v| (every operand replaced by its absolute value, |H| = diag(p) + p p^T) and
gamma = N + 2 sum_{l = 0..L} (width[l] + 1) + c + 8: the first-order sum of the lengths of the chained dot products (forward and
backward through every layer), of the H product and of the final sum over samples, plus the alpha v term.

Driver comparisons use DenseOp bound to the restated dense matrix with the same probes, and the tolerances of
tests/test_gpu_stencil.py::_close (rtol 1e-8, atol 1e-8 of the largest entry, fp64)."""

import ctypes as C

import numpy as np
import pytest
import torch

import _ggn_restatement as gr
from _guarded_ws import GuardedWs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib, cg, lanczos
    from matfree_extensions.operators import DenseOp, GgnMlpOp
    from matfree_extensions.util import bnn_util

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
PS = (1, 3, 5)
# (N, widths, loss, activation): every N, every width tuple, both losses meet at least once
CASES = [
    (1, (3, 7, 5, 3), "cross_entropy", "tanh"),
    (63, (3, 2), "cross_entropy", "tanh"),
    (64, (5, 64, 64, 2), "mse", "relu"),
    (65, (130, 4, 1, 4, 3), "cross_entropy", "relu"),
    (257, (3, 6, 1), "cross_entropy", "tanh"),
    (257, (3, 7, 5, 3), "mse", "tanh"),
    (65, (5, 64, 64, 2), "cross_entropy", "tanh"),
    (64, (130, 4, 1, 4, 3), "mse", "tanh"),
    (1, (3, 2), "mse", "relu"),
    (2081, (3, 2), "cross_entropy", "tanh"),
]
IDS = [f"N{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}" for c in CASES]


def T(x, dtype=torch.float64, grad=False):
    t = torch.tensor(np.asarray(x), dtype=dtype, device=DEV)
    return t.requires_grad_(True) if grad else t


def N64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def _close(got, want):
    return np.allclose(got, want, rtol=1e-8, atol=1e-8 * max(np.abs(want).max(), 1e-300))


_ops = {}


def _case(case, dtype):
    """operator, its tape upcast exactly to fp64 NumPy, theta as the device holds it -- built once per (case, dtype), never modified"""
    key = (case, dtype)
    if key not in _ops:
        n, widths, loss, activation = case
        rng = np.random.default_rng(n * 131 + len(widths))
        theta = T(rng.standard_normal(gr.param_count(widths)) * 0.7, dtype)
        x = T(rng.standard_normal((n, widths[0])), dtype)
        op = GgnMlpOp(x, theta, widths, activation=activation, loss=loss)
        tp = {"act": [N64(a) for a in op.tape["act"]], "dact": [None] + [N64(d) for d in op.tape["dact"][1:]],
              "prob": None if op.tape["prob"] is None else N64(op.tape["prob"])}
        _ops[key] = (op, tp, N64(op.theta))
    return _ops[key]


@pytest.fixture(scope="module", autouse=True)
def _release_the_operators_of_this_module():
    """The operators above stay alive for the whole module; afterwards they, and the cached device memory of this module's large
    guarded workspaces, go back to the driver: tests that count hipGraph replays rely on the caching allocator handing out the same
    addresses call after call, which takes longer to settle on a pool this module has fragmented."""
    yield
    _ops.clear()
    import gc

    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def gamma_of(n, widths):
    return n + 2 * sum(w + 1 for w in widths) + widths[-1] + 8


def _raw_apply(op, alpha, X, transpose=0, ldx=None, ldy=None, out=None):
    """mfx_op_apply through ctypes with explicit leading dimensions"""
    lib = _lib.get()
    p, n = X.shape[0], op.n
    desc = op.descriptor(op.constrain(alpha), X.dtype, n)
    ws = _lib.workspace(desc, n, 1, p, DEV)
    ldx, ldy = ldx or X.stride(0), ldy or n
    Y = torch.empty((p, ldy), dtype=X.dtype, device=DEV) if out is None else out
    _lib.check(lib.mfx_op_apply(C.byref(desc), _lib.ptr(X), ldx, _lib.ptr(Y), ldy, p, int(transpose), _lib.ptr(ws), ws.numel(),
                                _lib.stream_ptr(DEV)))
    return Y


def _raw_grad(op, alpha, L, R, g):
    lib = _lib.get()
    desc = op.descriptor(op.constrain(alpha), L.dtype, op.n)
    st = _lib.OpGrads()
    st.noise = None if g is None else g.data_ptr()
    ws = _lib.workspace(desc, op.n, 1, L.shape[0], DEV)
    return lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(L), L.stride(0), _lib.ptr(R), R.stride(0), L.shape[0], C.byref(st),
                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_apply_against_the_restatement(case, dtype, monkeypatch):
    guard = GuardedWs(poison=0xFF, busy=_lib._ws_busy)  # 0xFF: a partial sum that is read before it is written is a NaN
    monkeypatch.setattr(_lib, "_take", guard.take)
    n, widths, loss, _ = case
    op, tp, theta = _case(case, dtype)
    P, eps, gamma = op.n, eps_of(dtype), gamma_of(n, widths)
    rng = np.random.default_rng(7)
    alpha = T(0.37, dtype)
    for p in PS:
        X = T(rng.standard_normal((p, P)), dtype)
        Y = op(X, alpha)
        want = gr.apply_from_tape(tp, theta, widths, N64(X), N64(alpha), loss)
        s = gr.abs_apply_from_tape(tp, theta, widths, N64(X), N64(alpha), loss)
        err = np.abs(N64(Y) - want)
        ratio = float((err / np.maximum(gamma * eps * s, 1e-300)).max())
        print(f"apply {IDS[CASES.index(case)]} {dtype} p={p}: max err / (gamma eps s) = {ratio:.3g} (gamma = {gamma})")
        assert (err <= gamma * eps * s).all(), (p, ratio)
        # symmetric: transpose = 1 gives the same bits
        assert torch.equal(_raw_apply(op, alpha, X, transpose=1), Y)
        if widths[-1] == 1 and loss == "cross_entropy":  # softmax of one logit is 1 and H = 0: exactly alpha v
            assert torch.equal(Y, alpha * X)
    # leading dimensions larger than n: the gap is not written
    gap = 37
    Xp = torch.full((3, P + gap), float("nan"), dtype=dtype, device=DEV)
    Xp[:, :P] = X[:3] if X.shape[0] >= 3 else T(rng.standard_normal((3, P)), dtype)
    Yp = torch.full((3, P + 2 * gap), -777.0, dtype=dtype, device=DEV)
    _raw_apply(op, alpha, Xp, ldx=P + gap, ldy=P + 2 * gap, out=Yp)
    assert bool((Yp[:, P:] == -777.0).all())
    assert torch.equal(Yp[:, :P], op(Xp[:, :P].contiguous(), alpha))
    guard.verify()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_bit_reproducible_and_independent_of_the_probe_count(dtype):
    for case in (CASES[3], CASES[6], CASES[9]):
        op, _, _ = _case(case, dtype)
        X = T(np.random.default_rng(8).standard_normal((5, op.n)), dtype)
        alpha = T(0.37, dtype)
        Y = _raw_apply(op, alpha, X)
        assert torch.equal(Y, _raw_apply(op, alpha, X)) and bool(Y.abs().sum() > 0)
        for b in (0, 2, 4):  # first of a group, inside one, last of a ragged one (groups of 4 in fp32, 2 in fp64)
            assert torch.equal(_raw_apply(op, alpha, X[b : b + 1].contiguous())[0], Y[b])
        assert torch.equal(_raw_apply(op, alpha, X[1:4].contiguous()), Y[1:4])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", [CASES[0], CASES[6], CASES[7]], ids=[IDS[0], IDS[6], IDS[7]])
def test_shift_gradient_is_added_once(case, dtype, monkeypatch):
    guard = GuardedWs(poison=0xFF, busy=_lib._ws_busy)
    monkeypatch.setattr(_lib, "_take", guard.take)
    op, _, _ = _case(case, dtype)
    n, eps = op.n, eps_of(dtype)
    rng = np.random.default_rng(9)
    alpha = T(0.37, dtype)
    for batch in (1, 4, 33):
        L, R = T(rng.standard_normal((batch, n)), dtype), T(rng.standard_normal((batch, n)), dtype)
        for g0 in (0.0, 1.75):  # added to a non-zero initial value, it keeps that value
            g = T([g0], dtype)
            assert _raw_grad(op, alpha, L, R, g) == 0
            want = g0 + (N64(L) * N64(R)).sum()
            bound = batch * n * eps * (np.abs(N64(L)) * np.abs(N64(R))).sum()
            assert abs(float(g[0]) - want) <= bound, (batch, g0, float(g[0]), want, bound)
        g1, g2 = T([0.0], dtype), T([0.0], dtype)
        assert _raw_grad(op, alpha, L, R, g1) == 0 and _raw_grad(op, alpha, L, R, g2) == 0 and torch.equal(g1, g2)
    assert _raw_grad(op, alpha, L, R, None) == 0  # nothing asked for: MFX_OK, nothing written
    # through autograd: d/d alpha of sum(w o A(alpha) v) = w . v, d/d v = A w
    v, w = T(rng.standard_normal((3, n)), dtype, grad=True), T(rng.standard_normal((3, n)), dtype)
    a = T(0.37, dtype, grad=True)
    dv, da = torch.autograd.grad((w * op(v, a)).sum(), (v, a))
    assert da.shape == () and abs(float(da) - (N64(w) * N64(v)).sum()) <= 3 * n * eps * (np.abs(N64(w)) * np.abs(N64(v))).sum()
    assert torch.equal(dv, op(w, a.detach()))
    guard.verify()


# ---- drivers: the same calls on DenseOp bound to the restated dense matrix, the same probes (fp64) ----
def _driver_problem(which):
    """A: P = 86, k = 4, cross-entropy.  B: P = 15, k = P, mse on widths (2, 2, 3): a GGN with 15 well separated eigenvalues, so the
    full-depth recurrence does not break down (its smallest off-diagonal entry is 0.66 for these probes; a cross-entropy GGN of a net
    this small is rank deficient, the shift then has a multiple eigenvalue and the Krylov space ends before k = P)"""
    n, widths, k, loss = (65, (3, 7, 5, 3), 4, "cross_entropy") if which == "A" else (65, (2, 2, 3), 15, "mse")
    case = (n, widths, loss, "tanh")
    op, tp, theta = _case(case, torch.float64)
    G = gr.dense_matrix(tp, theta, widths, 0.0, loss)
    rng = np.random.default_rng(12)
    V = rng.standard_normal((3, op.n))
    return op, T(G), k, V, rng


def _dense_bound(G, alpha):
    return DenseOp().bind(G + alpha * torch.eye(G.shape[0], dtype=G.dtype, device=DEV))


@pytest.mark.parametrize("which", ["A", "B"])
def test_lanczos_forward_and_adjoint_against_the_dense_operator(which):
    op, G, k, V, rng = _driver_problem(which)
    P = op.n
    cot = (T(rng.standard_normal((3, k, P))), T(rng.standard_normal((3, k))), T(rng.standard_normal((3, k - 1))))
    outs = []
    for make in (lambda a: op.bind(a), lambda a: _dense_bound(G, a)):
        v, a = T(V, grad=True), T(0.37, grad=True)
        (Q, (diag, off)), _ = lanczos.tridiag(make(a), k, reortho="full")(v)
        loss = (Q * cot[0]).sum() + (diag * cot[1]).sum() + (off * cot[2]).sum()
        dv, da = torch.autograd.grad(loss, (v, a))
        outs.append([N64(t) for t in (Q, diag, off, dv, da)])
    for name, got, want in zip(("Q", "diag", "off", "dv", "dalpha"), *outs):
        assert _close(got, want), (which, name, float(np.abs(got - want).max()))


@pytest.mark.parametrize("which", ["A", "B"])
def test_slq_integrand_value_and_shift_derivative_against_the_dense_operator(which):
    op, G, k, V, _ = _driver_problem(which)
    outs = []
    for make in (lambda a: op.bind(a), lambda a: _dense_bound(G, a)):
        a = T(0.37, grad=True)
        val = lanczos.integrand_spd(torch.log, k, make(a))(T(V))
        (da,) = torch.autograd.grad(val.sum(), a)
        outs.append((N64(val), N64(da)))
    assert _close(outs[0][0], outs[1][0]) and _close(outs[0][1], outs[1][1]), outs


@pytest.mark.parametrize("which", ["A", "B"])
def test_cg_fixed_step_against_the_dense_operator(which):
    """Plain CG has no re-orthogonalisation: run to full depth (B, k = P) it amplifies a last-bit difference between two matvecs by
    the loss of orthogonality, which grows with the condition number.  In exact-order fp64 NumPy, on problem B, a relative 1e-16
    perturbation of the matvec moves the k = 15 iterate by 1e-4 .. 6e-4 at shift 0.37 (condition 231) and by 4e-12 .. 8e-11 at shift
    30 (condition 8.6).  Problem B therefore uses the shift 30, where the tolerance of _close measures the operator; problem A
    (k = 4) keeps 0.37, where the GGN part is the larger share of the operator."""
    op, G, k, V, _ = _driver_problem(which)
    a = T(0.37 if which == "A" else 30.0)
    x1, _ = cg.cg_fixed_step(k)(op.bind(a), T(V))
    x2, _ = cg.cg_fixed_step(k)(_dense_bound(G, a), T(V))
    assert _close(N64(x1), N64(x2)), float((x1 - x2).abs().max())


def test_calibration_loss_value_and_gradient_against_the_dense_operator():
    """N = 65, the reference MLP on d_in = 6, rank 10 and 10 probes; the same loss with a DenseOp of the restated matrix in the
    operator's place.  Autograd reaches log_alpha; a theta that requires grad raises."""
    init, apply = bnn_util.model_mlp(out_dims=3, activation="tanh")
    rng = np.random.default_rng(13)
    x = T(rng.standard_normal((65, 6)))
    theta = init(5, x)
    widths = init.widths(6)
    P = gr.param_count(widths)
    probes = T(rng.choice([-1.0, 1.0], size=(10, P)))
    tp = gr.tape(N64(theta), N64(x), widths, "tanh")
    G = T(gr.dense_matrix(tp, N64(theta), widths, 0.0))
    outs = []
    for operator in (None, lambda _op, alpha: _dense_bound(G, alpha)):
        loss = bnn_util.callibration_loss(apply, None, torch.exp, P, operator=operator)
        la = T(-1.0, grad=True)
        val = loss(la, theta, x, None, probes)
        (g,) = torch.autograd.grad(val, la)
        assert val.shape == () and g.shape == ()
        outs.append((float(val.detach()), float(g)))
    print("calibration loss (value, d/d log_alpha): GgnMlpOp", outs[0], "DenseOp", outs[1])
    assert _close(np.array(outs[0]), np.array(outs[1])), outs
    with pytest.raises(NotImplementedError, match="log_alpha only"):
        bnn_util.callibration_loss(apply, None, torch.exp, P)(T(-1.0), theta.clone().requires_grad_(True), x, None, probes)


def test_calibration_with_dense_logdet_against_the_slq_routes():
    """loss_calibration on the dense GGN (ggn_full + solver_logdet_dense) against the same loss on SLQ log-determinants: of the dense
    matrix (solver_logdet_slq) and of the matrix-free operator (solver_logdet_slq_implicit), integer keys (2 batches of 64 generated
    Rademacher probes).  Problem B of the driver tests at Lanczos depth P = 15: every quadratic form v^T log(A) v is then exact up to
    round-off and what is left is Hutchinson's sampling error, whose standard deviation for Rademacher probes is
    sqrt(2 sum_{i != j} M_ij^2 / num), M = log(A).  The logdets are compared at 4 such deviations (the seed is fixed: no flake), the
    losses at half that (the loss holds logdet / 2); the two SLQ routes run the same probes and agree as the driver tests do."""
    op, G, k, _, _ = _driver_problem("B")
    widths, n, num, batches = op.widths, op.n, 64, 2
    theta, x = op.theta, op.tape["act"][0]
    hot = torch.nn.functional.one_hot(torch.arange(x.shape[0], device=DEV) % 3, 3).double()
    la = T(np.log(0.37))
    full = bnn_util.ggn_full(loss_single=bnn_util.loss_training_mse_single,
                             model_fun=lambda th, xx: bnn_util.mlp_apply(th, xx, widths, "tanh"), param_unflatten=lambda v: v)
    A = full(torch.exp(la), theta, x, hot)
    assert _close(N64(A), N64(G) + 0.37 * np.eye(n))
    lam, U = np.linalg.eigh(N64(A))
    M = (U * np.log(lam)) @ U.T
    sigma = np.sqrt(2 * ((M**2).sum() - (np.diag(M) ** 2).sum()) / (num * batches))
    exact = float(bnn_util.solver_logdet_dense()(A))
    assert abs(exact - np.log(lam).sum()) <= 1e-10 * abs(exact)
    slq_dense = bnn_util.solver_logdet_slq(lanczos_rank=k, slq_num_samples=num, slq_num_batches=batches)
    slq_op = bnn_util.solver_logdet_slq_implicit(lanczos_rank=k, slq_num_samples=num, slq_num_batches=batches, N=n, x_like=theta)
    ld_dense, ld_op = float(slq_dense(A, 11)), float(slq_op(op.bind(torch.exp(la)), 11))
    print(f"logdet exact {exact:.6f}, slq dense {ld_dense:.6f}, slq operator {ld_op:.6f}, sigma {sigma:.4f}")
    assert abs(ld_dense - exact) <= 4 * sigma and abs(ld_op - exact) <= 4 * sigma
    assert _close(np.array(ld_op), np.array(ld_dense))
    losses = []
    for ggn_fun, logdet_fun, params in ((full, bnn_util.solver_logdet_dense(), ()), (full, slq_dense, (11,)),
                                        (lambda alpha, *_: op.bind(alpha), slq_op, (11,))):
        loss = bnn_util.loss_calibration(ggn_fun=ggn_fun, hyperparam_unconstrain=torch.exp, logdet_fun=logdet_fun)
        losses.append(float(loss(la, theta, x, hot, *params)))
    want = -(n / 2 * np.log(0.37) - 0.5 * 0.37 * float(theta @ theta) - 0.5 * exact)
    assert abs(losses[0] - want) <= 1e-10 * abs(want)
    assert abs(losses[1] - want) <= 2 * sigma and abs(losses[2] - want) <= 2 * sigma
