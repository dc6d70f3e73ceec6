"""The two Jacobian maps of an MLP (operators.MlpJacobian: J V and J^T U) and the linearised-Laplace predictive tier built on them, on
the GPU, against the NumPy restatement (tests/_mlp_jac_restatement.py) and against the same compositions on dense pieces.

Geometry of the kernels (csrc/mfx_ggn.hip): a workgroup takes tiles of 32 samples and a group of 4 (fp32) / 2 (fp64) probes; layers
past the input are one chunk of at most 64 units, the input is streamed in chunks of 64 columns.  J^T U uses at most 64 workgroups
along the samples (N > 2048: a workgroup walks more than one tile), J V at most 1024 (N > 32768).  Shapes: the N and widths of
tests/test_gpu_ggn.py -- N in {1, 63, 64, 65, 257}, 2081 for the tile loop of J^T U, widths with L = 1, a 64-wide layer, d_in = 130
(three chunks, the last ragged), one-unit layers and c = 1 -- and N = 32801 for the tile loop of J V; p in {1, 3, 5}.

Bounds of the maps.  The restatement is fed the device tape, upcast exactly, so only the kernels' arithmetic is judged:
|got - ref| <= gamma eps s entrywise, s the same chain with every operand replaced by its absolute value.  gamma is the first-order
sum of the lengths of the chained dot products.  J V: layer l adds a dot product of length width[l-1] against V_W_l, one of the same
length against W_l, and the bias: at most 2 (width[l-1] + 1) roundings on top of those its input carries; the slopes are one
multiplication per layer; summed over the layers and rounded up over all widths, gamma_f = 2 sum_{l = 0..L} (width[l] + 1) + 8.
J^T U: the products with W_l on the way down are at most as long, and an entry of the result is a sum over the N samples:
gamma_t = gamma_f + N.

Predictive tier (fp64): the mse net of widths (2, 2, 3) on 65 training points with the shift 30 (tests/test_gpu_ggn.py uses it for
its CG comparison: P = 15, a GGN that is not rank deficient, condition 8.6), CG with re-orthogonalisation at full depth P.
Comparisons with the same composition on DenseOp / a dense Jacobian use rtol 1e-8 and atol 1e-8 of the largest entry (_close)."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import _ggn_restatement as gr
import _mlp_jac_restatement as jr
from _guarded_ws import GuardedWs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib, cg
    from matfree_extensions.operators import DenseOp, GgnMlpOp, MlpJacobian
    from matfree_extensions.util import bnn_util

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
PS = (1, 3, 5)
# (N, widths, activation): the shapes of tests/test_gpu_ggn.py::CASES, and N = 32801 (1026 tiles) for the tile loop of J V
CASES = [
    (1, (3, 7, 5, 3), "tanh"),
    (63, (3, 2), "tanh"),
    (64, (5, 64, 64, 2), "relu"),
    (65, (130, 4, 1, 4, 3), "relu"),
    (257, (3, 6, 1), "tanh"),
    (257, (3, 7, 5, 3), "tanh"),
    (65, (5, 64, 64, 2), "tanh"),
    (64, (130, 4, 1, 4, 3), "tanh"),
    (1, (3, 2), "relu"),
    (2081, (3, 2), "tanh"),
    (32801, (3, 2), "tanh"),
]
IDS = [f"N{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}" for c in CASES]


def T(x, dtype=torch.float64, grad=False):
    t = torch.tensor(np.asarray(x), dtype=dtype, device=DEV)
    return t.requires_grad_(True) if grad else t


def N64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def _close(got, want):
    return np.allclose(got, want, rtol=1e-8, atol=1e-8 * max(np.abs(want).max(), 1e-300))


def gamma_f(widths):
    return 2 * sum(w + 1 for w in widths) + 8


def gamma_t(n, widths):
    return gamma_f(widths) + n


_jacs = {}


def _case(case, dtype):
    """the Jacobian, its tape upcast exactly to fp64 NumPy, theta as the device holds it -- built once per (case, dtype), never modified"""
    key = (case, dtype)
    if key not in _jacs:
        n, widths, activation = case
        rng = np.random.default_rng(n * 131 + len(widths))
        theta = T(rng.standard_normal(gr.param_count(widths)) * 0.7, dtype)
        x = T(rng.standard_normal((n, widths[0])), dtype)
        jac = MlpJacobian(x, theta, widths, activation=activation)
        tp = {"act": [N64(a) for a in jac.tape["act"]], "dact": [None] + [N64(d) for d in jac.tape["dact"][1:]]}
        _jacs[key] = (jac, tp, N64(jac.theta))
    return _jacs[key]


@pytest.fixture(scope="module", autouse=True)
def _release_the_tapes_of_this_module():
    """as tests/test_gpu_ggn.py: the tapes and the guarded workspaces go back to the driver when the module is done"""
    yield
    _jacs.clear()
    _predictive.clear()
    import gc

    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _raw_apply(jac, V, ldv=None, out=None):
    """mfx_mlp_jac_apply through ctypes with an explicit leading dimension and output"""
    p = V.shape[0]
    if out is None:
        out = torch.empty((p, jac.n_samples, jac.n_out), dtype=V.dtype, device=DEV)
    _lib.check(_lib.get().mfx_mlp_jac_apply(C.byref(jac.net), _lib.dtype_code(V.dtype), _lib.ptr(V), ldv or V.stride(0), p, _lib.ptr(out),
                                            _lib.stream_ptr(DEV)))
    return out


def _raw_t_apply(jac, U, ldy=None, out=None):
    """mfx_mlp_jac_t_apply through ctypes with an explicit leading dimension, its workspace from _lib's taker"""
    lib, p, code = _lib.get(), U.shape[0], _lib.dtype_code(U.dtype)
    ws = _lib.scratch(int(lib.mfx_mlp_jac_workspace_bytes(C.byref(jac.net), code, p)), DEV)
    ldy = ldy or jac.n_params
    Y = torch.empty((p, ldy), dtype=U.dtype, device=DEV) if out is None else out
    _lib.check(lib.mfx_mlp_jac_t_apply(C.byref(jac.net), code, _lib.ptr(U), p, _lib.ptr(Y), ldy, _lib.ptr(ws), ws.numel(),
                                       _lib.stream_ptr(DEV)))
    return Y


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_both_maps_against_the_restatement(case, dtype, monkeypatch):
    guard = GuardedWs(poison=0xFF, busy=_lib._ws_busy)  # 0xFF: a partial sum that is read before it is written is a NaN
    monkeypatch.setattr(_lib, "_take", guard.take)
    n, widths, _ = case
    jac, tp, theta = _case(case, dtype)
    P, c, eps = jac.n_params, widths[-1], eps_of(dtype)
    gf, gt = gamma_f(widths), gamma_t(n, widths)
    rng = np.random.default_rng(7)
    for p in PS:
        V, U = T(rng.standard_normal((p, P)), dtype), T(rng.standard_normal((p, n, c)), dtype)
        for name, got, want, s, gamma in (
            ("J V", jac.apply(V), jr.jac_apply_from_tape(tp, theta, widths, N64(V)), jr.abs_jac_apply_from_tape(tp, theta, widths, N64(V)), gf),
            ("J^T U", jac.t_apply(U), jr.jac_t_apply_from_tape(tp, theta, widths, N64(U)),
             jr.abs_jac_t_apply_from_tape(tp, theta, widths, N64(U)), gt),
        ):
            assert tuple(got.shape) == want.shape and got.dtype == dtype
            err = np.abs(N64(got) - want)
            ratio = float((err / np.maximum(gamma * eps * s, 1e-300)).max())
            print(f"{name} {IDS[CASES.index(case)]} {dtype} p={p}: max err / (gamma eps s) = {ratio:.3g} (gamma = {gamma})")
            assert (err <= gamma * eps * s).all(), (name, p, ratio)
        # one vector without the batch dimension: the same bits
        assert torch.equal(jac.apply(V[0]), jac.apply(V[:1])[0]) and torch.equal(jac.t_apply(U[0]), jac.t_apply(U[:1])[0])
    guard.verify()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", [CASES[3], CASES[6], CASES[9]], ids=[IDS[3], IDS[6], IDS[9]])
def test_leading_dimensions_and_the_end_of_the_output(case, dtype, monkeypatch):
    guard = GuardedWs(poison=0xFF, busy=_lib._ws_busy)
    monkeypatch.setattr(_lib, "_take", guard.take)
    n, widths, _ = case
    jac, _, _ = _case(case, dtype)
    P, c, gap, p = jac.n_params, widths[-1], 37, 3
    rng = np.random.default_rng(10)
    V, U = T(rng.standard_normal((p, P)), dtype), T(rng.standard_normal((p, n, c)), dtype)
    # ldv > P: the gap holds NaN, a read of it would reach the output; the output lies inside a larger buffer of sentinels
    Vp = torch.full((p, P + gap), float("nan"), dtype=dtype, device=DEV)
    Vp[:, :P] = V
    pad, size = 4096, p * n * c
    buf = torch.full((size + 2 * pad,), -777.0, dtype=dtype, device=DEV)
    out = _raw_apply(jac, Vp, ldv=P + gap, out=buf[pad : pad + size])
    assert bool((buf[:pad] == -777.0).all()) and bool((buf[pad + size :] == -777.0).all())
    assert torch.equal(out.reshape(p, n, c), jac.apply(V)) and bool(torch.isfinite(out).all())
    # ldy > P: the gap is not written
    Yp = torch.full((p, P + 2 * gap), -777.0, dtype=dtype, device=DEV)
    _raw_t_apply(jac, U, ldy=P + 2 * gap, out=Yp)
    assert bool((Yp[:, P:] == -777.0).all())
    assert torch.equal(Yp[:, :P], jac.t_apply(U))
    guard.verify()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_bit_reproducible_and_independent_of_the_probe_count(dtype):
    for case in (CASES[3], CASES[6], CASES[9]):
        n, widths, _ = case
        jac, _, _ = _case(case, dtype)
        rng = np.random.default_rng(8)
        V, U = T(rng.standard_normal((5, jac.n_params)), dtype), T(rng.standard_normal((5, n, widths[-1])), dtype)
        Y, O = _raw_t_apply(jac, U), _raw_apply(jac, V)
        assert torch.equal(Y, _raw_t_apply(jac, U)) and bool(Y.abs().sum() > 0)
        assert torch.equal(O, _raw_apply(jac, V)) and bool(O.abs().sum() > 0)
        for b in (0, 2, 4):  # first of a group, inside one, last of a ragged one (groups of 4 in fp32, 2 in fp64)
            assert torch.equal(_raw_t_apply(jac, U[b : b + 1].contiguous())[0], Y[b])
            assert torch.equal(_raw_apply(jac, V[b : b + 1].contiguous())[0], O[b])
        assert torch.equal(_raw_t_apply(jac, U[1:4].contiguous()), Y[1:4]) and torch.equal(_raw_apply(jac, V[1:4].contiguous()), O[1:4])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", [CASES[3], CASES[5], CASES[6]], ids=[IDS[3], IDS[5], IDS[6]])
def test_the_two_maps_are_transposes_and_each_is_the_backward_of_the_other(case, dtype):
    """<U, J V> and <J^T U, V>, summed in fp64 from the device results: the first is off by at most gamma_f eps <|U|, |J| |V|>, the
    second by at most gamma_t eps <|J|^T |U|, |V|>, which is the same number s; the fp64 sums add (N c + P) eps64 s at most."""
    n, widths, _ = case
    jac, tp, theta = _case(case, dtype)
    P, c, eps = jac.n_params, widths[-1], eps_of(dtype)
    rng = np.random.default_rng(11)
    V, U = T(rng.standard_normal((3, P)), dtype, grad=True), T(rng.standard_normal((3, n, c)), dtype, grad=True)
    JV, JtU = jac.apply(V), jac.t_apply(U)
    lhs, rhs = (N64(U) * N64(JV)).sum((1, 2)), (N64(JtU) * N64(V)).sum(1)
    s = (np.abs(N64(U)) * jr.abs_jac_apply_from_tape(tp, theta, widths, N64(V))).sum((1, 2))
    bound = (gamma_f(widths) + gamma_t(n, widths)) * eps * s + (n * c + P) * eps_of(torch.float64) * s
    print(f"adjointness {case} {dtype}: max |lhs - rhs| / bound = {float((np.abs(lhs - rhs) / bound).max()):.3g}")
    assert (np.abs(lhs - rhs) <= bound).all(), (lhs, rhs, bound)
    # autograd: the cotangent goes through the other kernel -- the same bits as calling it
    W, Z = T(rng.standard_normal((3, n, c)), dtype), T(rng.standard_normal((3, P)), dtype)
    (dV,) = torch.autograd.grad((W * JV).sum(), V)
    (dU,) = torch.autograd.grad((Z * JtU).sum(), U)
    assert torch.equal(dV, jac.t_apply(W)) and torch.equal(dU, jac.apply(Z))
    # ... and once more (the maps are linear: the backward of the backward is the map itself)
    (ddW,) = torch.autograd.grad((Z * jac.t_apply(W.requires_grad_(True))).sum(), W)
    assert torch.equal(ddW, jac.apply(Z))


def test_gradients_of_both_maps_in_fp64():
    """gradcheck where the number of inputs allows it (N = 63, widths (3, 2): 8 and 126 inputs); at N = 65, widths (5, 64, 64, 2)
    (4674 parameters) the explicit comparison with the restated transpose map, to the bound of that map."""
    jac, _, _ = _case(CASES[1], torch.float64)
    rng = np.random.default_rng(14)
    v = T(rng.standard_normal(jac.n_params), grad=True)
    u = T(rng.standard_normal((63, 2)), grad=True)
    assert torch.autograd.gradcheck(jac.apply, (v,), eps=1e-6, atol=1e-7, rtol=1e-7)
    assert torch.autograd.gradcheck(jac.t_apply, (u,), eps=1e-6, atol=1e-7, rtol=1e-7)
    case = CASES[6]
    n, widths, _ = case
    jac, tp, theta = _case(case, torch.float64)
    eps = eps_of(torch.float64)
    V, U = T(rng.standard_normal((2, jac.n_params)), grad=True), T(rng.standard_normal((2, n, 2)), grad=True)
    W, Z = T(rng.standard_normal((2, n, 2))), T(rng.standard_normal((2, jac.n_params)))
    (dV,) = torch.autograd.grad((W * jac.apply(V)).sum(), V)
    (dU,) = torch.autograd.grad((Z * jac.t_apply(U)).sum(), U)
    err = np.abs(N64(dV) - jr.jac_t_apply_from_tape(tp, theta, widths, N64(W)))
    assert (err <= gamma_t(n, widths) * eps * jr.abs_jac_t_apply_from_tape(tp, theta, widths, N64(W))).all()
    err = np.abs(N64(dU) - jr.jac_apply_from_tape(tp, theta, widths, N64(Z)))
    assert (err <= gamma_f(widths) * eps * jr.abs_jac_apply_from_tape(tp, theta, widths, N64(Z))).all()


@pytest.mark.parametrize("n,widths,loss,activation", [(65, (5, 64, 64, 2), "cross_entropy", "tanh"), (257, (3, 7, 5, 3), "mse", "tanh"),
                                                      (65, (130, 4, 1, 4, 3), "cross_entropy", "relu"), (64, (130, 4, 1, 4, 3), "mse", "tanh")],
                         ids=lambda v: str(v).replace(" ", ""))
def test_the_ggn_operator_is_the_two_maps_around_the_loss_hessian(n, widths, loss, activation):
    """op(V, alpha) against jac.t_apply(H o jac.apply(V)) + alpha V with jac = op.jacobian() (the operator's own tape) and H applied
    in torch from op.tape["prob"]: the fused pass and its two halves, fp64"""
    rng = np.random.default_rng(n * 131 + len(widths))
    theta, x = T(rng.standard_normal(gr.param_count(widths)) * 0.7), T(rng.standard_normal((n, widths[0])))
    op = GgnMlpOp(x, theta, widths, activation=activation, loss=loss)
    jac = op.jacobian()
    assert jac.tape["act"][0] is op.tape["act"][0] and jac.logits is op.tape["logits"]
    V, alpha = T(rng.standard_normal((3, op.n))), T(0.37)
    t = jac.apply(V)
    if loss == "cross_entropy":
        pr = op.tape["prob"][None]
        t = pr * t - pr * (pr * t).sum(-1, keepdim=True)
    got, want = N64(jac.t_apply(t) + alpha * V), N64(op(V, alpha))
    assert _close(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", [(65, (5, 64, 64, 2), "tanh"), (64, (130, 4, 1, 4, 3), "relu"), (2081, (3, 2), "tanh")],
                         ids=lambda c: f"N{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}")
def test_the_mse_operator_without_shift_has_the_bits_of_the_two_maps_back_to_back(case, dtype):
    """For mse the loss Hessian is the identity.  The fused kernel and the kernels of the two maps are separate code that forms every
    product and sum in the same order, so op(V, 0) and jac.t_apply(jac.apply(V)) must be the same bits: this pins that agreement.  The
    shapes: a ragged second tile, a three-chunk first layer with a width-1 layer, a workgroup that walks more than one tile; p = 5 is
    a ragged group."""
    n, widths, activation = case
    rng = np.random.default_rng(n * 131 + len(widths))
    theta, x = T(rng.standard_normal(gr.param_count(widths)) * 0.7, dtype), T(rng.standard_normal((n, widths[0])), dtype)
    op = GgnMlpOp(x, theta, widths, activation=activation, loss="mse")
    jac = op.jacobian()
    V = T(rng.standard_normal((5, op.n)), dtype)
    got, want = op(V, T(0.0, dtype)), jac.t_apply(jac.apply(V))
    assert bool(want.abs().sum() > 0) and torch.equal(got, want)


# ---- the predictive tier: native pieces against the same compositions on dense pieces (fp64) ----
class _DenseJac:
    """the interface of MlpJacobian over a dense (N, c, P) Jacobian: torch products on the device"""

    def __init__(self, J, logits):
        self.J, self.logits = J, logits
        self.n_samples, self.n_out, self.n_params = J.shape

    def rows(self, i0, i1):
        return _DenseJac(self.J[i0:i1], self.logits[i0:i1])

    def apply(self, V):
        return torch.einsum("ncp,bp->bnc", self.J, V)

    def t_apply(self, U):
        return torch.einsum("ncp,bnc->bp", self.J, U)


class _DenseGgn:
    """bind(alpha) -> DenseOp bound to the restated dense GGN + alpha I"""

    def __init__(self, G):
        self.G = G

    def bind(self, alpha):
        return DenseOp().bind(self.G + alpha * torch.eye(self.G.shape[0], dtype=self.G.dtype, device=DEV))


WIDTHS_B, N_B, SHIFT_B = (2, 2, 3), 65, 30.0
_predictive = {}


def _apply_like():
    """what the predictive functions read of model_mlp's apply: the widths and the activation"""

    def apply(theta, x):
        return bnn_util.mlp_apply(theta, x, WIDTHS_B, "tanh")

    apply.widths, apply.activation = (lambda d_in: WIDTHS_B), "tanh"
    return apply


def _problem_b(nstar):
    """the GGN operator over the training set, the restated dense GGN, theta, the test points; native and dense test Jacobians"""
    if nstar not in _predictive:
        rng = np.random.default_rng(N_B * 131 + len(WIDTHS_B))  # the operator of test_gpu_ggn's problem B
        theta, x = T(rng.standard_normal(gr.param_count(WIDTHS_B)) * 0.7), T(rng.standard_normal((N_B, 2)))
        op = GgnMlpOp(x, theta, WIDTHS_B, activation="tanh", loss="mse")
        tp = {"act": [N64(a) for a in op.tape["act"]], "dact": [None] + [N64(d) for d in op.tape["dact"][1:]], "prob": None}
        G = T(gr.dense_matrix(tp, N64(theta), WIDTHS_B, 0.0, "mse"))
        xs = T(np.random.default_rng(100 + nstar).standard_normal((nstar, 2)))
        jac = MlpJacobian(xs, theta, WIDTHS_B)
        Jd = torch.func.jacrev(lambda v: bnn_util.mlp_apply(v, xs, WIDTHS_B, "tanh"))(theta)
        _predictive[nstar] = (op, G, theta, x, xs, jac, _DenseJac(Jd, bnn_util.mlp_apply(theta, xs, WIDTHS_B, "tanh")))
    return _predictive[nstar]


@pytest.mark.parametrize("nstar", [33, 5], ids=["ragged-second-chunk", "one-short-chunk"])
def test_predictive_cov_operator_against_the_dense_routes(nstar):
    """Same solve (CG with re-orthogonalisation, P = 15 steps) on the native pieces and on DenseOp + a dense Jacobian: _close.  Against
    the dense inverse (bnn_util.predictive_cov) the DenseOp route is itself off by the error of 15 CG steps in fp64; the native route
    differs from it by rounding in the matvec only and is allowed 10 x that distance, both relative to the largest entry.  Measured on
    an MI355X: DenseOp route 5.52e-16 (N* = 33) and 2.27e-16 (N* = 5), native route 5.52e-16 and 3.41e-16."""
    op, G, theta, x, xs, jac, dense_jac = _problem_b(nstar)
    P = op.n
    solve = cg.cg_fixed_step_reortho(P)
    alpha = T(SHIFT_B)
    got = bnn_util.predictive_cov_operator(op, jac, solve=solve, chunk=32)(alpha)
    ref = bnn_util.predictive_cov_operator(_DenseGgn(G), dense_jac, solve=solve, chunk=32)(alpha)
    assert got.shape == (nstar, 3, 3)
    assert _close(N64(got), N64(ref)), float((got - ref).abs().max())
    model = lambda v, xx: bnn_util.mlp_apply(v, xx, WIDTHS_B, "tanh")  # noqa: E731
    full = bnn_util.ggn_full(loss_single=bnn_util.loss_training_mse_single, model_fun=model, param_unflatten=lambda v: v)
    inv = N64(bnn_util.predictive_cov(ggn_fun=full, model_fun=model, param_unflatten=lambda v: v, hyperparam_unconstrain=torch.exp)(
        T(math.log(SHIFT_B)), theta, x, torch.zeros(N_B, 3, dtype=torch.float64, device=DEV), xs))
    scale = np.abs(inv).max()
    d_dense, d_native = np.abs(N64(ref) - inv).max() / scale, np.abs(N64(got) - inv).max() / scale
    print(f"predictive_cov N*={nstar}: distance from the dense inverse / largest entry: DenseOp route {d_dense:.3g}, native {d_native:.3g}")
    assert d_dense <= 1e-8, "the yardstick itself: 15 re-orthogonalised CG steps on a 15 x 15 system of condition 8.6"
    assert d_native <= 10 * d_dense
    with pytest.raises(ValueError, match="chunk"):
        bnn_util.predictive_cov_operator(op, jac, chunk=0)


def test_joint_covariance_loglikelihood_and_sampler_against_the_dense_route():
    """predictive_posterior_loglikelihood (both logpdfs) and predictive_logit_sampler (explicit eps) on the native pieces against the same
    functions given the DenseOp-bound matvec and a torch.func Jacobian; N* = 3: the 9 x 9 joint covariance has full rank, which the
    Cholesky form needs (the Jacobian of this net has rank 13 of P = 15 at most: 12 x 12 is singular already), and its eigenvalues,
    3.6e-5 .. 0.15 in exact arithmetic, stay clear of the 1e-6 rule.  The joint covariance of 33 test points (99 x 99) is symmetric."""
    op, G, theta, _, xs, jac, dense_jac = _problem_b(3)
    P, solve, alpha = op.n, cg.cg_fixed_step_reortho(op.n), T(SHIFT_B)
    rng = np.random.default_rng(15)
    y, eps = T(rng.standard_normal((3, 3))), T(rng.standard_normal((6, 9)))
    routes = (dict(ggn_fun=op.bind(alpha)), dict(ggn_fun=_DenseGgn(G).bind(alpha), jacobian=lambda *_: dense_jac))
    outs = []
    for kw in routes:
        common = dict(model_apply=_apply_like(), unflatten=None, solve=solve, **kw)
        chol, info = bnn_util.predictive_posterior_loglikelihood(logpdf=bnn_util.logpdf_cholesky(), **common)(theta, xs, y)
        eigh, _ = bnn_util.predictive_posterior_loglikelihood(logpdf=bnn_util.logpdf_eigh(), **common)(theta, xs, y)
        samples = bnn_util.predictive_logit_sampler(num_samples=6, **common)(theta, xs, y, eps)
        assert info == {} and chol.shape == () and samples.shape == (6, 3, 3)
        outs.append((N64(chol), N64(eigh), N64(samples)))
    w = np.linalg.eigvalsh(N64(bnn_util._cov_matrix(bnn_util._joint_cov_vp(dense_jac, routes[1]["ggn_fun"], solve), dense_jac.logits.reshape(-1))))
    print(f"joint covariance N*=3: eigenvalues {w.min():.3g} .. {w.max():.3g}; logpdf cholesky {outs[0][0]:.12g} / {outs[1][0]:.12g}, "
          f"eigh {outs[0][1]:.12g} / {outs[1][1]:.12g}")
    assert w.min() > 1e-5, "the eigenvalues stay clear of logpdf_eigh's 1e-6 rule: both forms are the same density here"
    for name, got, want in zip(("logpdf_cholesky", "logpdf_eigh", "samples"), *outs):
        assert _close(got, want), (name, float(np.abs(got - want).max()))
    assert abs(outs[0][0] - outs[0][1]) <= 1e-8 * abs(outs[0][0])
    # a seed in place of eps: reproducible, and a different seed differs
    sampler = bnn_util.predictive_logit_sampler(model_apply=_apply_like(), unflatten=None, num_samples=3, solve=solve, ggn_fun=op.bind(alpha))
    s1, s2, s3 = sampler(theta, xs, y, 5), sampler(theta, xs, y, 5), sampler(theta, xs, y, 6)
    assert torch.equal(s1, s2) and not torch.equal(s1, s3)
    # symmetry of the joint covariance of 33 points, as the solver leaves it
    op, _, _, _, _, jac33, _ = _problem_b(33)
    Cj = N64(bnn_util._cov_matrix(bnn_util._joint_cov_vp(jac33, op.bind(alpha), solve), jac33.logits.reshape(-1)))
    assert Cj.shape == (99, 99) and np.abs(Cj - Cj.T).max() <= 1e-10 * np.abs(Cj).max()
    blocks = N64(bnn_util.predictive_cov_operator(op, jac33, solve=solve)(alpha))
    assert _close(np.stack([Cj[3 * i : 3 * i + 3, 3 * i : 3 * i + 3] for i in range(33)]), blocks)


def test_refusals():
    rng = np.random.default_rng(16)
    widths = (3, 4, 2)
    theta, x = T(rng.standard_normal(gr.param_count(widths))), T(rng.standard_normal((5, 3)))
    with pytest.raises(NotImplementedError, match="third derivatives"):
        MlpJacobian(x, theta.clone().requires_grad_(True), widths)
    with pytest.raises(NotImplementedError, match="third derivatives"):
        MlpJacobian(x.clone().requires_grad_(True), theta, widths)
    jac = MlpJacobian(x, theta, widths)
    with pytest.raises(TypeError, match="dtype"):
        jac.apply(torch.ones(2, jac.n_params, dtype=torch.float32, device=DEV))
    with pytest.raises(TypeError, match="dtype"):
        jac.t_apply(torch.ones(2, 5, 2, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="apply"):
        jac.apply(torch.ones(2, jac.n_params + 1, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="t_apply"):
        jac.t_apply(torch.ones(2, 4, 2, dtype=torch.float64, device=DEV))
    with pytest.raises(_lib.MfxError, match="no CPU fallback"):
        jac.apply(torch.ones(jac.n_params, dtype=torch.float64))
    # a layer wider than the kernels take: refused by the library, the limit named, nothing launched
    wide = (3, 65, 2)
    jw = MlpJacobian(x, T(rng.standard_normal(gr.param_count(wide))), wide)
    with pytest.raises(_lib.MfxError, match="limit 64"):
        jw.apply(torch.ones(1, jw.n_params, dtype=torch.float64, device=DEV))
    with pytest.raises(_lib.MfxError, match="limit 64"):
        jw.t_apply(torch.ones(1, 5, 2, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
