"""The exact GGN diagonal of an MLP (GgnMlpOp.diagonal, mfx_ggn_diag) and the diagonal-Laplace tier built on it, on the GPU, against
the NumPy restatement (tests/_ggn_diag_restatement.py), against the operator applied to the identity, and against dense pieces.

Geometry of the kernel (csrc/mfx_ggn.hip, k_ggn_diag_tiles): tiles of 32 samples, at most 64 workgroups along the samples (N > 2048: a
workgroup walks more than one tile) -- the tile size and the cap of k_ggn_tiles, so the N of tests/test_gpu_ggn.py::CASES stand as
they are: N in {1, 63, 64, 65, 257} and 2081, widths with L = 1, two 64-wide layers, d_in = 130 (three input chunks, the last
ragged), one-unit layers and c = 1.  The classes are dealt to the 4 (fp32) / 2 (fp64) waves of a workgroup round robin: c in
{1, 2, 3} leaves waves without a class, (65, (3, 4, 64)) makes every lane a class (16 / 32 rounds).  (65, (3, 7, 5, 3)) with the last
layer scaled by 50 has a softmax that is one-hot to rounding for four samples in ten: the variance m1 - m2^2 cancels there and the
clamp at 0 acts.  Every case runs with both losses and both dtypes.

Bound.  The restatement is fed the operator's own tape, upcast exactly, so only the kernel's arithmetic is judged:
|got - ref| <= gamma eps s entrywise, s the same chain with every operand replaced by its absolute value and the subtraction by an
addition.  gamma = 2 B + 2 c + N + 8 with B = sum_{l = 1..L} (width[l] + 1): going down, layer l costs a dot product of length
width[l] and the slope, at most B roundings in g by first order; g enters squared (m1) or twice (m2^2), which doubles that; the
two class sums add c each at most (the kernel adds them wave by wave, a different order of the same c terms); the sum over the
samples -- within a tile, over the tiles of a workgroup, over the workgroups -- has N non-zero terms; 8 covers p g, a^2, the product
with D and the subtraction."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import _ggn_diag_restatement as dr
import _ggn_restatement as gr
from _guarded_ws import GuardedWs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib
    from matfree_extensions.operators import DenseOp, GgnMlpOp
    from matfree_extensions.util import bnn_baselines, bnn_util

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
# (N, widths, activation, scale of the last layer): the shapes of tests/test_gpu_ggn.py::CASES, every lane a class, a saturated softmax
CASES = [
    (1, (3, 7, 5, 3), "tanh", 1.0),
    (63, (3, 2), "tanh", 1.0),
    (64, (5, 64, 64, 2), "relu", 1.0),
    (65, (130, 4, 1, 4, 3), "relu", 1.0),
    (257, (3, 6, 1), "tanh", 1.0),
    (257, (3, 7, 5, 3), "tanh", 1.0),
    (65, (5, 64, 64, 2), "tanh", 1.0),
    (64, (130, 4, 1, 4, 3), "tanh", 1.0),
    (1, (3, 2), "relu", 1.0),
    (2081, (3, 2), "tanh", 1.0),
    (65, (3, 4, 64), "tanh", 1.0),
    (65, (3, 7, 5, 3), "tanh", 50.0),
]
IDS = [f"N{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}" + ("-saturated" if c[3] != 1.0 else "") for c in CASES]


def T(x, dtype=torch.float64, grad=False):
    t = torch.tensor(np.asarray(x), dtype=dtype, device=DEV)
    return t.requires_grad_(True) if grad else t


def N64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def _close(got, want):
    return np.allclose(got, want, rtol=1e-8, atol=1e-8 * max(np.abs(want).max(), 1e-300))


def gamma_of(n, widths):
    return 2 * sum(w + 1 for w in widths[1:]) + 2 * widths[-1] + n + 8


_ops = {}


def _case(case, loss, dtype):
    """operator, its tape upcast exactly to fp64 NumPy, theta as the device holds it, the restated diagonal and its scale -- built
    once per (case, loss, dtype), never modified"""
    key = (case, loss, dtype)
    if key not in _ops:
        n, widths, activation, scale = case
        rng = np.random.default_rng(n * 131 + len(widths))
        theta = rng.standard_normal(gr.param_count(widths)) * 0.7
        theta[-(widths[-2] + 1) * widths[-1] :] *= scale
        x = T(rng.standard_normal((n, widths[0])), dtype)
        op = GgnMlpOp(x, T(theta, dtype), widths, activation=activation, loss=loss)
        tp = {"act": [N64(a) for a in op.tape["act"]], "dact": [None] + [N64(d) for d in op.tape["dact"][1:]],
              "prob": None if op.tape["prob"] is None else N64(op.tape["prob"])}
        th = N64(op.theta)
        _ops[key] = (op, tp, th, dr.diag_from_tape(tp, th, widths, loss), dr.abs_diag_from_tape(tp, th, widths, loss))
    return _ops[key]


@pytest.fixture(scope="module", autouse=True)
def _release_the_operators_of_this_module():
    """as tests/test_gpu_ggn.py: the tapes and the guarded workspaces go back to the driver when the module is done"""
    yield
    _ops.clear()
    import gc

    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("loss", gr.LOSSES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_diagonal_against_the_restatement_under_a_guarded_workspace(case, loss, dtype, monkeypatch):
    n, widths, _, scale = case
    op, _, _, want, s = _case(case, loss, dtype)
    eps, gamma = eps_of(dtype), gamma_of(n, widths)
    results = []
    for poison in (0xFF, 0x3C):  # 0xFF: a partial sum that is read before it is written is a NaN; 0x3C: a finite number
        guard = GuardedWs(poison=poison, busy=_lib._ws_busy)
        monkeypatch.setattr(_lib, "_take", guard.take)
        got = op.diagonal()
        guard.verify()  # the workspace is exactly mfx_ggn_diag_workspace_bytes: the bands around it are intact
        assert guard.handed_out == 1
        results.append(got)
    got = results[0]
    assert torch.equal(got, results[1]), "the result depends on what the workspace held"
    assert got.shape == (op.n,) and got.dtype == dtype
    assert bool(torch.isfinite(got).all()) and bool((got >= 0).all())
    err = np.abs(N64(got) - want)
    ratio = float((err / np.maximum(gamma * eps * s, 1e-300)).max())
    print(f"diagonal {IDS[CASES.index(case)]} {loss} {dtype}: max err / (gamma eps s) = {ratio:.3g} (gamma = {gamma}), "
          f"largest entry {want.max():.3g}")
    assert (err <= gamma * eps * s).all(), ratio
    if widths[-1] == 1 and loss == "cross_entropy":  # softmax of one logit is 1 and H = 0
        assert bool((got == 0).all())
    if scale != 1.0 and loss == "cross_entropy":
        pmax = N64(op.tape["prob"]).max(-1)  # in exact arithmetic 49 % of the samples have 1 - max p < 1e-6, 42 % < 2^-24
        assert (pmax > 1 - 1e-6).mean() >= 0.25, "the softmax of this case is meant to be one-hot to rounding for many samples"


def test_workspace_query_is_the_documented_size():
    lib = _lib.get()
    for case in (CASES[0], CASES[5], CASES[9]):
        for dtype in DTYPES:
            op = _case(case, "mse", dtype)[0]
            nblk = min(-(-case[0] // 32), 64)
            want = -(-nblk * op.n * (4 if dtype == torch.float32 else 8) // 256) * 256
            assert int(lib.mfx_ggn_diag_workspace_bytes(C.byref(op.net), _lib.dtype_code(dtype))) == want


@pytest.mark.parametrize("loss", gr.LOSSES)
@pytest.mark.parametrize("n,widths", [(257, (3, 7, 5, 3)), (65, (2, 2, 3))], ids=str)
def test_diagonal_is_the_diagonal_of_the_operator_applied_to_the_identity(n, widths, loss):
    """independent of the restatement, fp64: row b of op.bind(0)(I) is A e_b"""
    rng = np.random.default_rng(n * 131 + len(widths))
    theta, x = T(rng.standard_normal(gr.param_count(widths)) * 0.7), T(rng.standard_normal((n, widths[0])))
    op = GgnMlpOp(x, theta, widths, activation="tanh", loss=loss)
    P = op.n
    want = N64(torch.diagonal(op.bind(T(0.0))(torch.eye(P, dtype=torch.float64, device=DEV))))
    assert _close(N64(op.diagonal()), want), float(np.abs(N64(op.diagonal()) - want).max())
    alpha = T(0.37, grad=True)
    shifted = op.diagonal(alpha)
    assert _close(N64(shifted), want + 0.37)
    (g,) = torch.autograd.grad(shifted.sum(), alpha)
    assert float(g) == P
    assert torch.equal(op.diagonal(0.37), op.diagonal() + 0.37)
    assert torch.equal(bnn_baselines.exact_diagonal(theta, x, widths, likelihood="classification" if loss == "cross_entropy" else "regression"),
                       op.diagonal())


def _apply_like(widths):
    def apply(theta, x):
        return bnn_util.mlp_apply(theta, x, widths, "tanh")

    apply.widths, apply.activation = (lambda d_in: widths), "tanh"
    return apply


def test_python_tier_on_the_device_against_dense_pieces():
    """hutchinson_diagonal over the bound native operator against the same recursion on DenseOp of the restated matrix (explicit
    draws); callibration_loss_diagonal(exact=True) against the hand formula on the dense diagonal, value and log_alpha gradient;
    last_layer_ggn against the tail of op.diagonal().  fp64."""
    n, widths = 65, (3, 7, 5, 3)
    case = (n, widths, "tanh", 1.0)
    op, tp, th, want_diag, _ = _case(case, "cross_entropy", torch.float64)
    P = op.n
    theta, x = op.theta, op.tape["act"][0]
    G = T(gr.dense_matrix(tp, th, widths, 0.0))
    levels, samples = 3, 5
    draws = T(np.random.default_rng(21).standard_normal((levels, samples, P)))
    zero = T(0.0)
    dense = DenseOp().bind(G)
    outs = {}
    for mode in ("serial", "parallel"):
        outs[mode] = bnn_baselines.hutchinson_diagonal(op.bind(zero), theta, samples, draws, num_levels=levels, computation_type=mode)
        ref = bnn_baselines.hutchinson_diagonal(dense, theta, samples, draws, num_levels=levels, computation_type=mode)
        assert outs[mode].shape == (P,) and _close(N64(outs[mode]), N64(ref)), mode
        assert _close(N64(ref), dr.hutchinson_recursion(N64(G), N64(draws)))
    assert torch.equal(outs["serial"], outs["parallel"])  # a vector's bits do not depend on how many share the call

    # the calibration loss on the exact diagonal; the Hutchinson route with the same draws, on the native operator
    la = T(-1.0, grad=True)
    loss = bnn_util.callibration_loss_diagonal(_apply_like(widths), None, torch.exp, samples, levels, P, exact=True)
    val = loss(la, theta, x, None)
    (g,) = torch.autograd.grad(val, la)

    def hand(diag):
        lb = T(-1.0, grad=True)
        a = torch.exp(lb)
        cut = torch.where(diag < 1e-4, torch.zeros_like(diag), diag)
        v = -(torch.log(a) * P - a * torch.dot(theta, theta) - torch.log(cut + a).sum())
        return float(v.detach()), float(torch.autograd.grad(v, lb)[0])

    want = hand(T(np.diag(N64(G))))
    print("diagonal calibration loss (value, d/d log_alpha): exact", (float(val.detach()), float(g)), "dense", want)
    assert val.shape == () and _close(np.array([float(val.detach()), float(g)]), np.array(want))
    loss_h = bnn_util.callibration_loss_diagonal(_apply_like(widths), None, torch.exp, samples, levels, P, key=draws)
    val_h = loss_h(la, theta, x, None)
    (g_h,) = torch.autograd.grad(val_h, la)
    assert _close(np.array([float(val_h.detach()), float(g_h)]), np.array(hand(outs["serial"])))

    for likelihood, ls in (("classification", "cross_entropy"), ("regression", "mse")):
        o = _case(case, ls, torch.float64)[0]
        ll = bnn_baselines.last_layer_ggn(theta, x, widths, activation="tanh", likelihood=likelihood)
        m = (widths[-2] + 1) * widths[-1]
        assert ll.shape == (m, m) and ll.is_cuda
        assert _close(N64(torch.diagonal(ll)), N64(o.diagonal()[-m:]))
    torch.cuda.synchronize()


def test_refusals():
    rng = np.random.default_rng(22)
    x = T(rng.standard_normal((5, 3)))
    wide = (3, 65, 2)
    ow = GgnMlpOp(x, T(rng.standard_normal(gr.param_count(wide))), wide)
    with pytest.raises(_lib.MfxError, match="limit 64"):  # refused by the library, the limit named, nothing launched
        ow.diagonal()
    torch.cuda.synchronize()
    assert math.isfinite(float(GgnMlpOp(x, T(rng.standard_normal(8)), (3, 2)).diagonal().sum()))
