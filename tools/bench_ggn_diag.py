"""Times the exact GGN diagonal of an MLP (operators.GgnMlpOp.diagonal, mfx_ggn_diag, csrc/mfx_ggn.hip) at the shape of
tools/bench_ggn.py -- N = 8192, d_in = 784, c = 10, the reference MLP, fp32 -- in one process, the routes taking turns window by
window:

  (a) diagonal        op.diagonal(): c backward sweeps per sample, squared where they are produced
  (b) apply_c_probes  the operator applied to p = c probes: the nearest like-for-like on the existing kernel -- the same number of
                      backward sweeps per sample, plus the forward tangents the diagonal does not need
  (c) dense           torch.func: bnn_util.ggn_full(...).diagonal() on the first --dense-n samples (the (N, c, P) Jacobian and the
                      P x P matrix have to fit; 0 skips it), reported per call and scaled to N samples

Also checks (a) against the diagonal from (c) on those samples.  One JSON line; median [min, max] ms over the windows.

    python tools/bench_ggn_diag.py [--n 8192] [--d-in 784] [--classes 10] [--reps 7] [--dense-n 256]
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

from matfree_extensions.util import bnn_util  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dense-n", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ggn_diag.py needs a GPU"
    dev, dt = torch.device("cuda:0"), torch.float32
    gen = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(args.n, args.d_in, generator=gen).to(dev, dt)
    init, apply = bnn_util.model_mlp(out_dims=args.classes, activation="tanh")
    theta = init(1, x)
    widths = init.widths(args.d_in)
    P = theta.numel()
    op = bnn_util.ggn_operator(theta, x, widths, activation="tanh")
    V = torch.randn(args.classes, P, generator=gen).to(dev, dt)
    alpha = torch.tensor(0.0, device=dev, dtype=dt)
    res = {"tool": "bench_ggn_diag", "n": args.n, "widths": list(widths), "P": P, "dtype": "float32"}

    # the first call of each (code objects load, the scratch is allocated), then warm calls by the host clock around a synchronise
    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    routes = {"diagonal": op.diagonal, "apply_c_probes": lambda: op(V, alpha)}
    res["first_call_ms"] = {name: round(timed(fn, 1), 3) for name, fn in routes.items()}
    per_call = max(max(timed(fn, 5) for fn in routes.values()), 0.01)
    inner = int(min(2000, max(3, 400.0 / per_call)))  # windows of 0.4 s for the slower route
    res["calls_per_window"] = inner
    res["ms"] = windows({name: (fn, inner) for name, fn in routes.items()}, args.reps)
    res["diagonal_over_apply"] = round(res["ms"]["diagonal"][0] / res["ms"]["apply_c_probes"][0], 3)

    if args.dense_n > 0:
        nd = min(args.dense_n, args.n)
        xs = x[:nd].contiguous()
        hot = torch.nn.functional.one_hot(torch.arange(nd, device=dev) % args.classes, args.classes).to(dt)
        full = bnn_util.ggn_full(loss_single=bnn_util.loss_training_cross_entropy_single, model_fun=apply, param_unflatten=lambda v: v)

        def dense():
            return torch.diagonal(full(alpha, theta, xs, hot)).clone()

        want = dense()
        got = bnn_util.ggn_operator(theta, xs, widths, activation="tanh").diagonal()
        res["dense_n"] = nd
        res["diagonal_relerr_vs_dense"] = float((got - want).abs().max() / want.abs().max())
        res["ms"].update(windows({"dense": (dense, 1)}, min(args.reps, 3)))
        res["dense_ms_scaled_to_n"] = round(res["ms"]["dense"][0] * args.n / nd, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
