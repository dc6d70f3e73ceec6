"""Times the two Jacobian maps of an MLP (operators.MlpJacobian, csrc/mfx_ggn.hip: J V and J^T U) and the per-point predictive
covariance built on them (bnn_util.predictive_cov_operator) against the same maps written as torch.func jvp / vjp over
bnn_util.mlp_apply, in one process, the two routes taking turns window by window.  Shape: N* = 8192, d_in = 784, c = 10, the reference
MLP, fp32, p = 10 for the maps; 256 test points against 8192 training points for the covariance (chunks of 32 points, the
reference's 20 re-orthogonalised CG steps on the native GGN operator in both routes: only the Jacobian maps differ).

One JSON line; median [min, max] ms over the windows.

    python tools/bench_mlp_jac.py [--n 8192] [--d-in 784] [--classes 10] [--probes 10] [--test-points 256] [--reps 7]
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ggn import windows  # noqa: E402
from matfree_extensions.operators import MlpJacobian  # noqa: E402
from matfree_extensions.util import bnn_util  # noqa: E402


class TorchFuncJacobian:
    """the interface of MlpJacobian through torch.func jvp / vjp over mlp_apply, one vector at a time"""

    def __init__(self, x, theta, widths, activation):
        self.x, self.theta, self.widths, self.activation = x, theta, widths, activation
        self.n_samples, self.n_out, self.n_params = x.shape[0], widths[-1], theta.numel()
        self.logits = self._f(theta)

    def _f(self, th):
        return bnn_util.mlp_apply(th, self.x, self.widths, self.activation)

    def rows(self, i0, i1):
        return TorchFuncJacobian(self.x[i0:i1], self.theta, self.widths, self.activation)

    def apply(self, V):
        return torch.stack([torch.func.jvp(self._f, (self.theta,), (v,))[1] for v in V])

    def t_apply(self, U):
        vjp = torch.func.vjp(self._f, self.theta)[1]
        return torch.stack([vjp(u)[0] for u in U])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d-in", type=int, default=784)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--probes", type=int, default=10)
    ap.add_argument("--test-points", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mlp_jac.py needs a GPU"
    dev, dt = torch.device("cuda:0"), torch.float32
    gen = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(args.n, args.d_in, generator=gen).to(dev, dt)
    init, _ = bnn_util.model_mlp(out_dims=args.classes, activation="tanh")
    theta = init(1, x)
    widths = init.widths(args.d_in)
    P = theta.numel()
    jac, ref = MlpJacobian(x, theta, widths), TorchFuncJacobian(x, theta, widths, "tanh")
    V = torch.randn(args.probes, P, generator=gen).to(dev, dt)
    U = torch.randn(args.probes, args.n, args.classes, generator=gen).to(dev, dt)
    res = {"tool": "bench_mlp_jac", "n": args.n, "widths": list(widths), "P": P, "probes": args.probes, "dtype": "float32"}

    def relerr(a, b):
        return float((a - b).abs().max() / b.abs().max())

    res["apply_relerr_vs_torch"] = relerr(jac.apply(V), ref.apply(V))
    res["t_apply_relerr_vs_torch"] = relerr(jac.t_apply(U), ref.t_apply(U))
    for _ in range(3):  # warm-up of both routes
        jac.apply(V), jac.t_apply(U), ref.apply(V), ref.t_apply(U)
    res["apply_ms"] = windows({"mlp_jacobian": (lambda: jac.apply(V), 200), "torch_jvp": (lambda: ref.apply(V), 30)}, args.reps)
    res["t_apply_ms"] = windows({"mlp_jacobian": (lambda: jac.t_apply(U), 200), "torch_vjp": (lambda: ref.t_apply(U), 30)}, args.reps)
    res["apply_flops"] = res["t_apply_flops"] = 2 * args.n * P * args.probes  # 2 flops per parameter, sample and probe
    res["apply_tflops"] = round(res["apply_flops"] / (res["apply_ms"]["mlp_jacobian"][0] * 1e-3) / 1e12, 3)
    res["t_apply_tflops"] = round(res["t_apply_flops"] / (res["t_apply_ms"]["mlp_jacobian"][0] * 1e-3) / 1e12, 3)

    # the per-point predictive covariance of the first test points against all training points
    m = args.test_points
    xs = torch.randn(m, args.d_in, generator=gen).to(dev, dt)
    op = bnn_util.ggn_operator(theta, x, widths, activation="tanh")
    alpha = torch.tensor(0.1, device=dev, dtype=dt)
    native = bnn_util.predictive_cov_operator(op, MlpJacobian(xs, theta, widths))
    through_torch = bnn_util.predictive_cov_operator(op, TorchFuncJacobian(xs, theta, widths, "tanh"))
    res["test_points"] = m
    res["predictive_cov_relerr_vs_torch"] = relerr(native(alpha), through_torch(alpha))
    res["predictive_cov_ms"] = windows({"mlp_jacobian": (lambda: native(alpha), 1), "torch_jvp_vjp": (lambda: through_torch(alpha), 1)},
                                       args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
