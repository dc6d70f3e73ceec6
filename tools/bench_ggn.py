"""Times the matrix-free GGN operator of an MLP (operators.GgnMlpOp, csrc/mfx_ggn.hip) against the same operator written as
torch.func jvp + vjp behind CallbackOp, in one process, the two routes taking turns window by window: the apply on p probes and one calibration value-and-gradient
(bnn_util.callibration_loss: rank 10, 10 probes).  Shape: N = 8192, d_in = 784, c = 10, the reference MLP, fp32.

Also prints the achieved fraction of the tape-byte roofline of the apply: the tape, N (d_in + 2 sum of hidden widths + c) elements,
read once per probe group at the measured HBM copy rate (6.29 TB/s).  One JSON line; median [min, max] ms over the windows.

    python tools/bench_ggn.py [--n 8192] [--d-in 784] [--classes 10] [--probes 10] [--reps 7]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))

from matfree_extensions.operators import CallbackOp  # noqa: E402
from matfree_extensions.util import bnn_util  # noqa: E402

HBM_BYTES_PER_S = 6.29e12


def windows(routes, reps):
    """routes: {name: (fn, calls per window)}.  The routes take turns, window by window; -> {name: [median, min, max] ms per call}"""
    out = {name: [] for name in routes}
    for _ in range(reps):
        for name, (fn, inner) in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / inner * 1e3)
    return {name: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)] for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d-in", type=int, default=784)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--probes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ggn.py needs a GPU"
    dev, dt = torch.device("cuda:0"), torch.float32
    gen = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(args.n, args.d_in, generator=gen).to(dev, dt)
    init, apply = bnn_util.model_mlp(out_dims=args.classes, activation="tanh")
    theta = init(1, x)
    widths = init.widths(args.d_in)
    P = theta.numel()
    op = bnn_util.ggn_operator(theta, x, widths, activation="tanh")

    def f(th):
        return apply(th, x)

    def torch_matvec(v, alpha):  # one vector: J^T H J v + alpha v through jvp and vjp (softmax Hessian in closed form)
        logits, jv = torch.func.jvp(f, (theta,), (v,))
        p = torch.softmax(logits, -1)
        hjv = p * jv - p * (p * jv).sum(-1, keepdim=True)
        (out,) = torch.func.vjp(f, theta)[1](hjv)
        return out + alpha * v

    cb = CallbackOp(torch_matvec)
    V = torch.randn(args.probes, P, generator=gen).to(dev, dt)
    alpha = torch.tensor(0.1, device=dev, dtype=dt)
    y_native = op(V, alpha)
    y_torch = torch.stack([torch_matvec(v, alpha) for v in V])
    relerr = float((y_native - y_torch).abs().max() / y_torch.abs().max())
    res = {"tool": "bench_ggn", "n": args.n, "widths": list(widths), "P": P, "probes": args.probes, "dtype": "float32",
           "apply_relerr_vs_torch": relerr}
    for _ in range(3):  # warm-up of both routes
        op(V, alpha)
        [torch_matvec(v, alpha) for v in V]
    res["apply_ms"] = windows({"ggn_op": (lambda: op(V, alpha), 200),  # about half a second per window
                               "torch_jvp_vjp": (lambda: [torch_matvec(v, alpha) for v in V], 30)}, args.reps)
    tape_bytes = args.n * (args.d_in + 2 * sum(widths[1:-1]) + args.classes) * 4
    groups = (args.probes + 3) // 4
    res["tape_bytes"] = tape_bytes
    res["roofline_ms_tape_once_per_group"] = round(groups * tape_bytes / HBM_BYTES_PER_S * 1e3, 5)
    res["apply_fraction_of_tape_roofline"] = round(res["roofline_ms_tape_once_per_group"] / res["apply_ms"]["ggn_op"][0], 5)
    res["apply_flops"] = 4 * args.n * P * args.probes  # forward and backward, 2 flops per parameter, sample and probe each
    res["apply_tflops"] = round(res["apply_flops"] / (res["apply_ms"]["ggn_op"][0] * 1e-3) / 1e12, 3)

    probes = torch.randint(0, 2, (10, P), generator=gen).to(dev, dt) * 2 - 1

    def calibration(operator):
        loss = bnn_util.callibration_loss(apply, None, torch.exp, P, operator=operator)

        def run():
            la = torch.tensor(-2.0, device=dev, dtype=dt, requires_grad=True)
            val = loss(la, theta, x, None, probes)
            (g,) = torch.autograd.grad(val, la)
            return float(val.detach()), float(g)

        return run

    native, callback = calibration(None), calibration(lambda _op, a: cb.bind(a))
    res["calibration_value_grad"] = {"ggn_op": native(), "torch_jvp_vjp": callback()}
    res["calibration_ms"] = windows({"ggn_op": (native, 10), "torch_jvp_vjp": (callback, 1)}, args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
