"""The posterior mean's cross-covariance matvec y = K(X_new, X) v forward alone against forward + backward (fp32, RBF, ARD
lengthscale, p = 1), over the shapes of DESIGN.md section 3.3c.  Backward = the transposed matvec (d/dv) and the VJP sweeps for the
lengthscale, outputscale, X_new and X -- everything RbfGramOp.cross_apply's backward can be asked for -- plus, separately, the
X_new-only request of acquisition optimisation.  Times are medians of --reps runs, each bracketed by synchronisations.

  python tools/bench_cross_grad.py [--reps R] [--shapes m,n,d;m,n,d;...]

One JSON line per shape on stdout.  The log of a run on the MI355X is kept under profiles/."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "experiments-lanczos-adjoints_amd"))
import torch  # noqa: E402
from matfree_extensions.operators import RbfGramOp  # noqa: E402

SHAPES = [(16, 131072, 8), (32768, 131072, 8), (4096, 53500, 20), (1024, 100000, 90)]


def inv_softplus(v):
    return math.log(math.expm1(v))


def median_ms(fn, reps):
    fn()  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", type=str, default="", help="m,n,d;m,n,d;... (default: the four of DESIGN.md 3.3c)")
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in args.shapes.split(";")] if args.shapes else SHAPES
    dev = torch.device("cuda:0")
    for m, n, d in shapes:
        g = torch.Generator().manual_seed(7)
        X = torch.randn((n, d), generator=g).to(dev) / math.sqrt(d / 8)
        xn0 = torch.randn((m, d), generator=g).to(dev) / math.sqrt(d / 8)
        v0 = torch.randn((n,), generator=g).to(dev)
        ybar = torch.randn((m,), generator=g).to(dev)
        raw = [torch.tensor(r, dtype=torch.float32, device=dev) for r in ([inv_softplus(1.5)] * d, inv_softplus(1.0), -2.0)]

        def forward():
            with torch.no_grad():
                RbfGramOp(X).cross_apply(xn0, v0, *raw)

        def fwd_bwd(all_inputs):
            xn = xn0.clone().requires_grad_(True)
            if all_inputs:
                Xg, v = X.clone().requires_grad_(True), v0.clone().requires_grad_(True)
                params = [raw[0].clone().requires_grad_(True), raw[1].clone().requires_grad_(True), raw[2]]
                wrt = [xn, Xg, v, params[0], params[1]]
            else:
                Xg, v, params, wrt = X, v0, raw, [xn]
            y = RbfGramOp(Xg).cross_apply(xn, v, *params)
            torch.autograd.grad((ybar * y).sum(), wrt)

        t_fwd = median_ms(forward, args.reps)
        t_all = median_ms(lambda: fwd_bwd(True), args.reps)
        t_xn = median_ms(lambda: fwd_bwd(False), args.reps)
        print(json.dumps({"m": m, "n": n, "d": d, "p": 1, "dtype": "fp32", "kernel": "rbf", "ard": True,
                          "forward_ms": round(t_fwd, 3), "fwd_bwd_all_ms": round(t_all, 3), "fwd_bwd_xnew_ms": round(t_xn, 3),
                          "bwd_all_over_fwd": round((t_all - t_fwd) / t_fwd, 2),
                          "bwd_xnew_over_fwd": round((t_xn - t_fwd) / t_fwd, 2)}), flush=True)


if __name__ == "__main__":
    main()
