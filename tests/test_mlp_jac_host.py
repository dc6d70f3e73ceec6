"""CPU-side checks of the MLP Jacobian maps and the predictive tier (no GPU): the NumPy restatement the GPU tests measure against, tied
to torch.func; the three entry points declared, bound, exported and documented; the Python surface, which has no CPU fallback; the
refusals of the C-ABI under the sanitizers in a stand-alone program; the dense pieces of the predictive tier on the CPU."""

import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _ggn_restatement as gr
import _mlp_jac_restatement as jr
from matfree_extensions import _lib
from matfree_extensions.operators import GgnMlpOp, MlpJacobian
from matfree_extensions.util import bnn_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mfx_mlp_jac_workspace_bytes", "mfx_mlp_jac_apply", "mfx_mlp_jac_t_apply"]
F64 = torch.float64


def _problem(widths, N, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(gr.param_count(widths)) * 0.7, rng.standard_normal((N, widths[0]))


@pytest.mark.parametrize("activation", gr.ACTIVATIONS)
@pytest.mark.parametrize("widths", [(3, 7, 5, 3), (3, 2), (4, 6, 1, 3), (2, 2, 1)], ids=str)
def test_restatement_is_the_torch_func_jacobian_and_its_transpose(widths, activation):
    theta, x = _problem(widths, 9)
    tp = gr.tape(theta, x, widths, activation, "mse")
    J = torch.func.jacrev(lambda v: bnn_util.mlp_apply(v, torch.tensor(x), widths, activation))(torch.tensor(theta)).numpy()  # (N, c, P)
    rng = np.random.default_rng(1)
    V, U = rng.standard_normal((3, len(theta))), rng.standard_normal((4, 9, widths[-1]))
    JV, JtU = jr.jac_apply_from_tape(tp, theta, widths, V), jr.jac_t_apply_from_tape(tp, theta, widths, U)
    want_JV, want_JtU = np.einsum("ncp,bp->bnc", J, V), np.einsum("ncp,bnc->bp", J, U)
    assert JV.shape == (3, 9, widths[-1]) and JtU.shape == (4, len(theta))
    assert np.abs(JV - want_JV).max() <= 1e-13 * max(np.abs(want_JV).max(), 1.0)
    assert np.abs(JtU - want_JtU).max() <= 1e-13 * max(np.abs(want_JtU).max(), 1.0)
    assert np.abs(jr.dense_jacobian(tp, theta, widths) - J).max() <= 1e-13 * max(np.abs(J).max(), 1.0)
    # <U, J V> = <J^T U, V>
    lhs, rhs = np.einsum("bnc,anc->ba", U, JV), JtU @ V.T
    assert np.abs(lhs - rhs).max() <= 1e-12 * np.abs(lhs).max()
    # the scales dominate
    assert (np.abs(JV) <= jr.abs_jac_apply_from_tape(tp, theta, widths, V) * (1 + 1e-12)).all()
    assert (np.abs(JtU) <= jr.abs_jac_t_apply_from_tape(tp, theta, widths, U) * (1 + 1e-12)).all()
    # the GGN of the mse loss is J^T J: the composition of the two maps is the restated operator
    G = gr.dense_matrix(tp, theta, widths, 0.0, "mse")
    JtJ = jr.jac_t_apply_from_tape(tp, theta, widths, jr.jac_apply_from_tape(tp, theta, widths, np.eye(len(theta))))
    assert np.abs(JtJ - G).max() <= 1e-12 * np.abs(G).max()


def test_the_three_entry_points_are_declared_bound_exported_and_documented():
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.get()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mfx.h"
        assert name in _lib.SYMBOLS, f"{name} is not in _lib.SYMBOLS"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert re.search(r"`" + name + r"`", integration), f"{name} has no row in INTEGRATION.md"
        decl = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*)\);", header, flags=re.M).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name
    # additive: the version and the table of operator kinds are the parent's
    assert re.search(r"#define MFX_VERSION 201\b", header) and lib.mfx_version() == 201
    assert "MFX_OP_GGN = 5 }" in header


def test_python_surface_exists_and_refuses_cpu_tensors():
    widths = (3, 4, 2)
    theta, x = _problem(widths, 5)
    th, xt = torch.tensor(theta), torch.tensor(x)
    jac = MlpJacobian(xt, th, widths, activation="relu")
    assert (jac.n_params, jac.n_samples, jac.n_out) == (gr.param_count(widths), 5, 2)
    want = gr.tape(theta, x, widths, "relu", "mse")
    assert jac.logits.shape == (5, 2) and np.allclose(jac.logits.numpy(), want["logits"], rtol=1e-13, atol=1e-13)
    assert jac.tape["prob"] is None and jac.net.prob is None and jac.net.nsamples == 5 and list(jac.net.width)[:3] == list(widths)
    for call, arg in ((jac.apply, torch.ones(jac.n_params, dtype=F64)), (jac.apply, torch.ones(2, jac.n_params, dtype=F64)),
                      (jac.t_apply, torch.ones(5, 2, dtype=F64)), (jac.t_apply, torch.ones(3, 5, 2, dtype=F64))):
        with pytest.raises(_lib.MfxError, match="no CPU fallback"):
            call(arg)
    # GgnMlpOp's refusals, with its message
    with pytest.raises(NotImplementedError, match="third derivatives"):
        MlpJacobian(xt, th.clone().requires_grad_(True), widths)
    with pytest.raises(NotImplementedError, match="third derivatives"):
        MlpJacobian(xt.clone().requires_grad_(True), th, widths)
    with pytest.raises(ValueError):
        MlpJacobian(xt, th, widths, activation="gelu")
    with pytest.raises(ValueError, match="parameters"):
        MlpJacobian(xt, th[:-1], widths)
    with pytest.raises(ValueError, match="widths"):
        MlpJacobian(xt[:, :2], th, widths)
    # over an operator's tape: the tensors are shared; a slice is a view of the same memory
    op = GgnMlpOp(xt, th, widths, activation="relu")
    shared = op.jacobian()
    assert shared.theta is op.theta and shared.logits is op.tape["logits"]
    assert all(a is b for a, b in zip(shared.tape["act"], op.tape["act"])) and shared.tape["dact"][1] is op.tape["dact"][1]
    assert shared.net.prob is None and op.net.prob == op.tape["prob"].data_ptr()
    part = shared.rows(1, 4)
    assert part.n_samples == 3 and part.net.nsamples == 3 and part.logits.shape == (3, 2)
    assert part.tape["act"][0].data_ptr() == op.tape["act"][0][1:].data_ptr() and part.net.act[1] == op.tape["act"][1][1:].data_ptr()
    assert all(t.is_contiguous() for t in part.tape["act"])
    with pytest.raises(ValueError, match="rows"):
        shared.rows(3, 6)
    for name in ("logpdf_cholesky", "logpdf_eigh", "predictive_cov", "predictive_cov_operator", "predictive_posterior_loglikelihood",
                 "predictive_logit_sampler"):
        assert callable(getattr(bnn_util, name)), name


def test_host_argument_checks_of_the_entry_points_under_the_sanitizers():
    """`make asan` builds the host code of libmfx under AddressSanitizer + UndefinedBehaviorSanitizer and, with the same flags,
    tests/cabi/cabi_jac_checks.cpp: every bad argument of the three entry points is refused with its status code before any launch,
    and the workspace query is pure host arithmetic.  A stand-alone program, run here without a GPU."""
    csrc = os.path.join(ROOT, "experiments-lanczos-adjoints_amd", "csrc")
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists(clang)):
        pytest.skip("needs make, hipcc and the ROCm clang")
    rt = subprocess.run([clang, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("the sanitizer runtime is not installed")
    build = subprocess.run(["make", "-C", csrc, "asan", "-j4"], capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
    chk = subprocess.run([os.path.join(csrc, "asan", "cabi_jac_checks")], capture_output=True, text=True, timeout=300)
    assert chk.returncode == 0 and "cabi_jac_checks ok" in chk.stdout, chk.stdout[-2000:] + chk.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in chk.stderr and "runtime error:" not in chk.stderr, chk.stderr[-3000:]


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return torch.tensor((Q * np.linspace(0.5, 3.0, n)) @ Q.T)


def test_logpdfs_are_the_gaussian_density_and_take_one_batched_call():
    n = 6
    Cm = _spd(n, 2)
    rng = np.random.default_rng(3)
    y, mean = torch.tensor(rng.standard_normal(n)), torch.tensor(rng.standard_normal(n))
    calls = []

    def cov(V):
        calls.append(tuple(V.shape))
        return V @ Cm.T

    want = float(torch.distributions.MultivariateNormal(mean, covariance_matrix=Cm).log_prob(y))
    for make in (bnn_util.logpdf_cholesky, bnn_util.logpdf_eigh):
        calls.clear()
        val, info = make()(y, mean=mean, cov=cov)
        assert info == {} and calls == [(n, n)]
        assert abs(float(val) - want) <= 1e-12 * abs(want), (make.__name__, float(val), want)
    # a non-symmetric callable: row b of the batched call is the COLUMN b of the matrix
    A = torch.tensor(rng.standard_normal((n, n)))
    assert torch.allclose(bnn_util._cov_matrix(lambda V: V @ A.T, mean), A, rtol=0, atol=1e-15)
    # the w < 1e-6 rules of logpdf_eigh: such a direction counts 0 in the log-determinant and 0 in the Mahalanobis norm
    w = torch.tensor([2.0, 0.5, 1e-7, -1e-3], dtype=F64)
    Q, _ = np.linalg.qr(rng.standard_normal((4, 4)))
    Q = torch.tensor(Q)
    Cs = (Q * w) @ Q.T
    r = torch.tensor(rng.standard_normal(4))
    val, _ = bnn_util.logpdf_eigh()(r, mean=torch.zeros(4, dtype=F64), cov=lambda V: V @ Cs.T)
    z = Q.T @ r
    want = -(math.log(2.0) + math.log(0.5)) / 2 - 0.5 * float(z[0] ** 2 / 2.0 + z[1] ** 2 / 0.5) - 2 * math.log(2 * math.pi)
    assert abs(float(val) - want) <= 1e-9 * abs(want)


class _DenseJac:
    """the interface of MlpJacobian over a dense (N, c, P) Jacobian, torch ops (runs anywhere)"""

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
    def __init__(self, G):
        self.G = G

    def bind(self, alpha):
        return self.G + alpha * torch.eye(self.G.shape[0], dtype=self.G.dtype)


def _exact_solve(A, B):
    return torch.linalg.solve(A, B.T).T, {}


def test_predictive_tier_on_dense_pieces_is_the_dense_baseline():
    """predictive_cov (inverse of ggn_full, jacrev) against predictive_cov_operator, the joint covariance of the log-likelihood and
    the sampler, all fed a dense Jacobian, a dense GGN and an exact solve: the compositions themselves, on the CPU."""
    widths, N, Ns = (2, 2, 3), 20, 7
    theta, x = _problem(widths, N, seed=4)
    xs = np.random.default_rng(5).standard_normal((Ns, 2))
    th, xt, xst = torch.tensor(theta), torch.tensor(x), torch.tensor(xs)
    model = lambda v, xx: bnn_util.mlp_apply(v, xx, widths, "tanh")  # noqa: E731
    full = bnn_util.ggn_full(loss_single=bnn_util.loss_training_mse_single, model_fun=model, param_unflatten=lambda v: v)
    la = torch.tensor(math.log(0.37), dtype=F64)
    want = bnn_util.predictive_cov(ggn_fun=full, model_fun=model, param_unflatten=lambda v: v, hyperparam_unconstrain=torch.exp)(
        la, th, xt, torch.zeros(N, 3, dtype=F64), xst)
    assert want.shape == (Ns, 3, 3)
    tps = gr.tape(theta, xs, widths, "tanh", "mse")
    jac = _DenseJac(torch.tensor(jr.dense_jacobian(tps, theta, widths)), torch.tensor(tps["logits"]))
    G = torch.tensor(gr.dense_matrix(gr.tape(theta, x, widths, "tanh", "mse"), theta, widths, 0.0, "mse"))
    for chunk in (32, 3, 1):  # one short chunk; ragged; one point each
        got = bnn_util.predictive_cov_operator(_DenseGgn(G), jac, solve=_exact_solve, chunk=chunk)(torch.exp(la))
        assert got.shape == (Ns, 3, 3) and torch.allclose(got, want, rtol=1e-10, atol=1e-12)
    # the joint covariance: its diagonal blocks are the per-point covariances; log-likelihood and sampler use it as documented
    A = G + 0.37 * torch.eye(len(theta), dtype=F64)
    Jf = jac.J.reshape(Ns * 3, -1)
    Cj = Jf @ torch.linalg.solve(A, Jf.T)
    assert torch.allclose(torch.stack([Cj[3 * i : 3 * i + 3, 3 * i : 3 * i + 3] for i in range(Ns)]), want, rtol=1e-10, atol=1e-12)
    _, apply = bnn_util.model_mlp(out_dims=3)
    y = torch.tensor(np.random.default_rng(6).standard_normal((Ns, 3)))
    common = dict(model_apply=apply, unflatten=None, ggn_fun=A, solve=_exact_solve, jacobian=lambda *_: jac)
    # rank min(P, N* c) = 15 < 21: the Cholesky form needs full rank, so the eigh form here
    val, _ = bnn_util.predictive_posterior_loglikelihood(logpdf=bnn_util.logpdf_eigh(), **common)(th, xst, y)
    w, v = torch.linalg.eigh(0.5 * (Cj + Cj.T))
    keep = w >= 1e-6
    r = v.T @ (y.reshape(-1) - jac.logits.reshape(-1))
    want_val = -torch.log(w[keep]).sum() / 2 - 0.5 * (r[keep] ** 2 / w[keep]).sum() - Ns * 3 / 2 * math.log(2 * math.pi)
    assert abs(float(val) - float(want_val)) <= 1e-9 * abs(float(want_val))
    eps = torch.tensor(np.random.default_rng(7).standard_normal((4, Ns * 3)))
    samples = bnn_util.predictive_logit_sampler(num_samples=4, **common)(th, xst, y, eps)
    F = (v[:, keep] / torch.sqrt(w[keep])) @ v[:, keep].T  # the reference's quirk: 1 / w under the root
    assert samples.shape == (4, Ns, 3)
    assert torch.allclose(samples.reshape(4, -1), jac.logits.reshape(-1) + eps @ F.T, rtol=1e-8, atol=1e-8)
    with pytest.raises(ValueError, match="chunk"):
        bnn_util.predictive_cov_operator(_DenseGgn(G), jac, chunk=0)
