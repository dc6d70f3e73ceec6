"""CPU-side checks of the matrix-free GGN operator of an MLP (no GPU): the NumPy restatement the GPU tests measure against, tied to
torch.func; the ctypes mirror of struct mfx_ggn_net; the refusals of the C-ABI, which all come before any launch (the descriptor's
pointers are never dereferenced); the theta layout and the tape of the Python layer."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _ggn_restatement as gr
from matfree_extensions import _lib
from matfree_extensions.operators import GgnMlpOp, RowShardedOp
from matfree_extensions.util import bnn_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(widths, N, seed=0):
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal(gr.param_count(widths)) * 0.7
    x = rng.standard_normal((N, widths[0]))
    return theta, x


def _torch_dense(theta, x, widths, activation, loss, alpha):
    """sum_i J_i^T H_i J_i + alpha I from torch.func.jacrev and hessian, fp64 on the CPU"""
    th, xt = torch.tensor(theta), torch.tensor(x)

    def f(v):
        return bnn_util.mlp_apply(v, xt, widths, activation)

    single = bnn_util.loss_training_cross_entropy_single if loss == "cross_entropy" else bnn_util.loss_training_mse_single
    y = torch.zeros(len(x), widths[-1], dtype=torch.float64)
    y[:, 0] = 1.0
    J = torch.func.jacrev(f)(th)
    H = torch.func.vmap(torch.func.hessian(single, argnums=0))(f(th), y)
    return (torch.einsum("nci,ncd,ndj->ij", J, H, J) + alpha * torch.eye(len(theta), dtype=torch.float64)).numpy()


@pytest.mark.parametrize("loss", gr.LOSSES)
@pytest.mark.parametrize("activation", gr.ACTIVATIONS)
@pytest.mark.parametrize("widths", [(3, 7, 5, 3), (3, 2), (4, 6, 1, 3)], ids=str)
def test_restated_dense_matrix_is_the_torch_func_ggn(widths, activation, loss):
    theta, x = _problem(widths, 9)
    alpha = 0.37
    tp = gr.tape(theta, x, widths, activation, loss)
    A = gr.dense_matrix(tp, theta, widths, alpha, loss)
    want = _torch_dense(theta, x, widths, activation, loss, alpha)
    assert np.abs(A - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(A - A.T).max() <= 1e-13 * np.abs(A).max()
    # ggn_full, the dense baseline of bnn_util, is the same matrix
    single = bnn_util.loss_training_cross_entropy_single if loss == "cross_entropy" else bnn_util.loss_training_mse_single
    full = bnn_util.ggn_full(loss_single=single, model_fun=lambda th, xx: bnn_util.mlp_apply(th, xx, widths, activation),
                             param_unflatten=lambda v: v)
    hot = torch.nn.functional.one_hot(torch.arange(9) % widths[-1], widths[-1]).double()  # labels that sum to 1: H = diag(p) - p p^T
    got = full(torch.tensor(alpha, dtype=torch.float64), torch.tensor(theta), torch.tensor(x), hot)
    assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # the scale |A| |v| dominates |A v|
    V = np.random.default_rng(1).standard_normal((3, len(theta)))
    assert (np.abs(gr.apply_from_tape(tp, theta, widths, V, alpha, loss)) <= gr.abs_apply_from_tape(tp, theta, widths, V, alpha, loss) * (1 + 1e-12)).all()


def test_one_class_cross_entropy_is_exactly_alpha_times_identity():
    widths = (3, 6, 1)
    theta, x = _problem(widths, 11)
    tp = gr.tape(theta, x, widths, "tanh")
    assert np.array_equal(tp["prob"], np.ones((11, 1)))
    assert np.array_equal(gr.dense_matrix(tp, theta, widths, 0.3), 0.3 * np.eye(len(theta)))


def test_ggn_net_mirror_matches_the_header_as_compiled():
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    body = header[header.index("typedef struct mfx_ggn_net {") : header.index("} mfx_ggn_net;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)(?:\[[^\]]*\])?;", body)
    names = [f[0] for f in _lib.GgnNet._fields_]
    assert names == fields
    fmt = " ".join(["%zu"] * (len(names) + 1))
    args = ", ".join(["sizeof(mfx_ggn_net)"] + [f"offsetof(mfx_ggn_net, {n})" for n in names])
    prog = f'#include <stdio.h>\n#include <stddef.h>\n#include "mfx.h"\nint main(void){{printf("{fmt}\\n", {args});return 0;}}'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.GgnNet)] + [getattr(_lib.GgnNet, n).offset for n in names]
    values = dict(re.findall(r"(MFX_(?:OP|GGN)_[A-Z0-9_]+) = (\d+)", header))
    assert values["MFX_OP_GGN"] == "5" == str(_lib.OP_GGN)
    assert (values["MFX_GGN_CROSS_ENTROPY"], values["MFX_GGN_MSE"]) == ("0", "1") == (str(_lib.GGN_CROSS_ENTROPY), str(_lib.GGN_MSE))
    assert re.search(r"#define MFX_GGN_MAX_LAYERS 8\b", header) and _lib.GGN_MAX_LAYERS == 8


def _net(widths=(3, 7, 5, 3), N=9, loss=_lib.GGN_CROSS_ENTROPY, nlayers=None, **null):
    net = _lib.GgnNet()
    L = len(widths) - 1 if nlayers is None else nlayers
    net.nlayers, net.loss, net.nsamples = L, loss, N
    for l, w in enumerate(widths[: _lib.GGN_MAX_LAYERS + 1]):
        net.width[l] = w
    net.theta = 64  # never dereferenced
    for l in range(min(max(L, 0), _lib.GGN_MAX_LAYERS)):
        net.act[l] = 64
        if l >= 1:
            net.dact[l] = 64
    net.prob = 64
    for name, idx in null.items():
        if idx is True:
            setattr(net, name, None)
        else:
            getattr(net, name)[idx] = None
    return net


def _desc(net, n=None, nrows=0, noise=64, dtype=_lib.MFX_F64):
    desc = _lib.Operator()
    desc.kind, desc.dtype = _lib.OP_GGN, dtype
    widths = [net.width[l] for l in range(max(min(net.nlayers, 8), 0) + 1)] if net is not None else [1, 1]
    desc.n = gr.param_count(widths) if n is None else n
    desc.noise = noise
    desc.ctx = ctypes.addressof(net) if net is not None else None
    desc.nrows = nrows
    desc._keep = net
    return desc


def test_refusals_come_before_any_launch():
    lib = _lib.get()
    fake = ctypes.c_void_p(64)
    big = 1 << 40

    def apply(desc):
        return lib.mfx_op_apply(ctypes.byref(desc), fake, desc.n, fake, desc.n, 1, 0, fake, big, None)

    def vjp(desc, g=None):
        if g is None:
            g = _lib.OpGrads()
            g.noise = 64
        return lib.mfx_op_vjp_params(ctypes.byref(desc), fake, desc.n, fake, desc.n, 1, ctypes.byref(g), fake, big, None)

    def forward(desc):
        return lib.mfx_lanczos_forward(ctypes.byref(desc), fake, desc.n, 2, 1, fake, fake, fake, fake, fake, big, None)

    invalid = {
        "null ctx": _desc(None, n=8),
        "null theta": _desc(_net(theta=True)),
        "null noise": _desc(_net(), noise=None),
        "null act[0]": _desc(_net(act=0)),
        "null act[2]": _desc(_net(act=2)),
        "null dact[1]": _desc(_net(dact=1)),
        "null prob": _desc(_net(prob=True)),
        "nlayers 0": _desc(_net(nlayers=0), n=8),
        "nlayers 9": _desc(_net(widths=(2,) * 9, nlayers=9), n=8),
        "width 0": _desc(_net(widths=(3, 0, 5, 3)), n=8),
        "width -1": _desc(_net(widths=(3, 7, 5, -1)), n=8),
        "N 0": _desc(_net(N=0)),
        "n != P": _desc(_net(), n=85),
        "loss 2": _desc(_net(loss=2)),
        "loss -1": _desc(_net(loss=-1)),
    }
    for what, desc in invalid.items():
        for call in (apply, vjp, forward):
            assert call(desc) == -1, what
            assert "GGN" in lib.mfx_last_error().decode(), what
    # mse needs no prob; dact[0] is never required
    assert vjp(_desc(_net(loss=_lib.GGN_MSE, prob=True)), _lib.OpGrads()) == 0
    # sizes outside the range of the kernels, the limit named; the issue's range is inside it
    for call in (apply, vjp, forward):
        assert call(_desc(_net(widths=(3, 65, 3)))) == -2 and "limit 64" in lib.mfx_last_error().decode()
        assert call(_desc(_net(widths=(3, 7, 65)))) == -2 and "limit 64" in lib.mfx_last_error().decode()
        assert call(_desc(_net(widths=(65537, 7, 3)))) == -2 and "limit 65536" in lib.mfx_last_error().decode()
    assert vjp(_desc(_net(widths=(4096, 64, 64, 64))), _lib.OpGrads()) == 0
    # a row block
    for call in (apply, vjp):
        assert call(_desc(_net(), nrows=8)) == -2 and "row block" in lib.mfx_last_error().decode()
    # gradient fields the kind does not have
    for field in ("x", "dense_a", "val"):
        g = _lib.OpGrads()
        g.noise = 64
        setattr(g, field, 64)
        assert vjp(_desc(_net()), g) == -2 and "third derivatives" in lib.mfx_last_error().decode(), field
    # the row-sharded drivers
    cm = _lib.Comm()
    cm.rank, cm.world, cm.nloc = 0, 1, 512
    cm.allreduce_sum = _lib.ALLREDUCE_T(lambda *a: 0)
    cm.allgather = _lib.ALLGATHER_T(lambda *a: 0)
    net = _net(widths=(7, 64))  # P = 512, inside the kernels' range
    whole = _desc(net)
    assert whole.n == 512
    assert lib.mfx_lanczos_forward_sharded(ctypes.byref(whole), ctypes.byref(cm), fake, 512, 2, 1, fake, fake, fake, fake, fake, big,
                                           None) == -2
    assert "row sharding a GGN" in lib.mfx_last_error().decode()
    assert lib.mfx_arnoldi_forward_sharded(ctypes.byref(whole), ctypes.byref(cm), fake, 512, 2, 1, 1, fake, fake, fake, fake, fake,
                                           fake, big, None) == -2
    assert lib.mfx_pcg_solve_sharded(ctypes.byref(whole), ctypes.byref(cm), fake, 512, 512, 1, None, 0, None, None, 3, 0, 0.0, 0.0, 0,
                                     fake, fake, None, fake, big, None) == -2
    assert "row sharding a GGN" in lib.mfx_last_error().decode()
    # the element access of the partial Cholesky refuses the kind, as for CSR
    assert lib.mfx_partial_cholesky(ctypes.byref(whole), 2, 0, 0, fake, fake, fake, fake, big, None) == -2
    # no gradient asked for: MFX_OK, nothing launched
    assert vjp(_desc(_net()), _lib.OpGrads()) == 0
    # more vectors than a grid holds: refused by name at the entry point, not as a launch failure
    ok = _desc(_net())
    assert lib.mfx_op_apply(ctypes.byref(ok), fake, ok.n, fake, ok.n, 65536, 0, fake, big, None) == -2
    assert "p too large" in lib.mfx_last_error().decode()


def test_workspace_is_the_partial_sums_of_the_apply():
    lib = _lib.get()
    dense = _lib.Operator()
    dense.kind, dense.dtype, dense.n = _lib.OP_DENSE, _lib.MFX_F64, 86
    base = int(lib.mfx_workspace_bytes(ctypes.byref(dense), 86, 1, 3)) - 256
    # N = 65 is three tiles of 32 samples: 3 workgroups x 3 probes x 86 values
    assert int(lib.mfx_workspace_bytes(ctypes.byref(_desc(_net(N=65))), 86, 1, 3)) == base + (3 * 3 * 86 * 8 + 255) // 256 * 256
    # at most 64 workgroups along the samples
    assert int(lib.mfx_workspace_bytes(ctypes.byref(_desc(_net(N=10**6))), 86, 1, 3)) == base + (64 * 3 * 86 * 8 + 255) // 256 * 256


def test_model_mlp_theta_layout_round_trips():
    init, apply = bnn_util.model_mlp(out_dims=4, activation="tanh")
    x = torch.randn(6, 2, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    theta = init(3, x)
    widths = init.widths(6)
    assert widths == (6, 50, 50, 5, 5, 4) and theta.shape == (gr.param_count(widths),) and theta.dtype == torch.float64
    layers = bnn_util.mlp_unflatten(theta, widths)
    assert [tuple(l["kernel"].shape) for l in layers] == [(6, 50), (50, 50), (50, 5), (5, 5), (5, 4)]
    assert all(bool((l["bias"] == 0).all()) for l in layers) and all(float(l["kernel"].std()) > 0 for l in layers)
    # bias first, then the kernel, layer by layer; the restatement splits the same way
    for layer, (b, W) in zip(layers, gr.split(theta.numpy(), widths)):
        assert np.array_equal(layer["bias"].numpy(), b) and np.array_equal(layer["kernel"].numpy(), W)

    def tree_model(params, xx):
        a = xx.reshape(xx.shape[0], -1)
        for l, layer in enumerate(params):
            a = a @ layer["kernel"] + layer["bias"]
            a = torch.tanh(a) if l + 1 < len(params) else a
        return a

    vec, unflatten, apply_vec = bnn_util.vectorize_nn(tree_model, layers)
    assert torch.equal(vec, theta)
    assert all(torch.equal(a["kernel"], b["kernel"]) and torch.equal(a["bias"], b["bias"]) for a, b in zip(unflatten(vec), layers))
    assert torch.equal(apply_vec(vec, x), apply(theta, x))
    assert np.allclose(apply(theta, x).numpy(), gr.tape(theta.numpy(), x.numpy(), widths, "tanh")["logits"], rtol=1e-13, atol=1e-13)
    # metrics, reference semantics
    logits = torch.tensor([[2.0, 0.0], [0.0, 1.0], [3.0, 1.0]], dtype=torch.float64)
    hot = torch.tensor([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    probs = torch.softmax(logits, -1)
    assert float(bnn_util.metric_accuracy(probs=probs, labels_hot=hot)) == pytest.approx(1 / 3)
    assert float(bnn_util.metric_confidence(probs=probs)) == pytest.approx(float(probs.max(-1).values.mean()))
    assert float(bnn_util.metric_nll(logits=logits, labels_hot=hot)) == pytest.approx(float(-(hot * torch.log(probs)).sum()))
    assert float(bnn_util.metric_nll(logits=logits, labels_hot=hot, sum_or_mean_fun=torch.mean)) == pytest.approx(
        float(-(hot * torch.log(probs)).sum() / 3))
    assert float(bnn_util.slq_log_clipped()(torch.tensor([0.0, 1e-30, 2.0], dtype=torch.float64)).sum()) == pytest.approx(np.log(2.0))
    M = torch.diag(torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64))
    assert float(bnn_util.solver_logdet_dense()(M)) == pytest.approx(np.log(8.0))


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-13)])
@pytest.mark.parametrize("loss", gr.LOSSES)
@pytest.mark.parametrize("activation", gr.ACTIVATIONS)
def test_tape_of_the_python_layer_is_the_restated_tape(activation, loss, dtype, tol):
    widths = (5, 7, 1, 4, 3)
    theta, x = _problem(widths, 13, seed=3)
    th, xt = torch.tensor(theta, dtype=dtype), torch.tensor(x, dtype=dtype)
    op = GgnMlpOp(xt, th, widths, activation=activation, loss=loss)
    assert op.size() == gr.param_count(widths) == op.n
    want = gr.tape(th.double().numpy(), xt.double().numpy(), widths, activation, loss)
    assert len(op.tape["act"]) == len(want["act"]) == 4 and op.tape["dact"][0] is None
    for l in range(4):
        assert np.abs(op.tape["act"][l].double().numpy() - want["act"][l]).max() <= tol * max(1.0, np.abs(want["act"][l]).max())
        if l >= 1:
            assert np.abs(op.tape["dact"][l].double().numpy() - want["dact"][l]).max() <= tol
    if loss == "cross_entropy":
        assert np.abs(op.tape["prob"].double().numpy() - want["prob"]).max() <= tol
    else:
        assert op.tape["prob"] is None and op.net.prob is None
    # the descriptor: kind 5, ctx at the operator's own struct, alpha in the noise slot, its gradient wired to grads.noise
    alpha = torch.tensor(0.5, dtype=dtype)
    (a1,) = op.constrain(alpha)
    desc = op.descriptor((a1,), dtype, op.n)
    assert (desc.kind, desc.n, desc.ctx, desc.noise) == (5, op.n, ctypes.addressof(op.net), a1.data_ptr())
    assert op.net.nlayers == 4 and op.net.nsamples == 13 and list(op.net.width)[:5] == list(widths)
    assert op.net.act[0] == op.tape["act"][0].data_ptr() and op.net.dact[0] is None and op.net.dact[3] == op.tape["dact"][3].data_ptr()
    s, (g,) = op.new_grads(a1)
    assert s.noise == g.data_ptr() and g.shape == (1,) and s.val is None and s.x is None
    with pytest.raises(TypeError, match="dtype"):
        op.descriptor((a1.to(torch.float64 if dtype == torch.float32 else torch.float32),), dtype, op.n)


def test_python_layer_refusals():
    widths = (3, 4, 2)
    theta, x = _problem(widths, 5)
    th, xt = torch.tensor(theta), torch.tensor(x)
    with pytest.raises(NotImplementedError, match="third derivatives"):
        GgnMlpOp(xt, th.clone().requires_grad_(True), widths)
    with pytest.raises(NotImplementedError, match="third derivatives"):
        GgnMlpOp(xt.clone().requires_grad_(True), th, widths)
    for bad in (dict(activation="gelu"), dict(loss="hinge")):
        with pytest.raises(ValueError):
            GgnMlpOp(xt, th, widths, **bad)
    with pytest.raises(ValueError, match="parameters"):
        GgnMlpOp(xt, th[:-1], widths)
    with pytest.raises(ValueError, match="x_train"):
        GgnMlpOp(xt[:, :2], th, widths)
    with pytest.raises(ValueError):
        GgnMlpOp(xt, th, (3,) + (2,) * 9)
    with pytest.raises(NotImplementedError, match="row sharding"):
        RowShardedOp(GgnMlpOp(xt, th, widths), comm=None)
    assert isinstance(bnn_util.ggn_operator(th, xt, widths, activation=torch.relu, loss="mse"), GgnMlpOp)
    init, apply = bnn_util.model_mlp(out_dims=2, activation="relu")
    loss = bnn_util.callibration_loss(apply, None, torch.exp, gr.param_count(init.widths(3)))
    with pytest.raises(NotImplementedError, match="log_alpha only"):
        loss(torch.tensor(0.0, dtype=torch.float64), init(0, xt).requires_grad_(True), xt, None, 1)


def test_calibration_loss_rebuilds_the_tape_for_another_theta():
    """The loss keeps its operator only while the same two tensor objects come back.  Temporaries (a fresh clone per call, whose id()
    the allocator may hand out again) must each get their own tape."""
    init, apply = bnn_util.model_mlp(out_dims=2, activation="tanh")
    x = torch.randn(5, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    thetas = [init(seed, x) for seed in range(4)]
    seen = []

    class Stop(Exception):
        pass

    def operator(op, alpha):  # stands where the bound matvec is made: records the tape in use, then ends the call (no GPU here)
        seen.append(op)
        raise Stop

    loss = bnn_util.callibration_loss(apply, None, torch.exp, thetas[0].numel(), operator=operator)
    la = torch.tensor(0.0, dtype=torch.float64)
    for th in thetas:
        with pytest.raises(Stop):
            loss(la, th.clone(), x, None, 1)  # a temporary: freed after the call
        assert torch.equal(seen[-1].theta, th)
        want = gr.tape(th.numpy(), x.numpy(), init.widths(3), "tanh")
        assert np.allclose(seen[-1].tape["prob"].numpy(), want["prob"], rtol=1e-13, atol=1e-13)
    assert len({id(op) for op in seen}) == 4
    # the same two objects again: the tape is kept
    for _ in range(2):
        with pytest.raises(Stop):
            loss(la, thetas[2], x, None, 1)
    assert seen[-1] is seen[-2] and torch.equal(seen[-1].theta, thetas[2])
