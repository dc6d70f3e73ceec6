"""Pathwise GP posterior samples (operators.RandomFeatures, gp_util.PathwisePosterior) at BASELINE config 4's shape:
n = 131 072 training points, d = 8, S = 64 samples, m in {1024, 4096} random features, fp32.

  evaluate        RandomFeatures.evaluate at the n training points (mfx_rff_apply), against ONE Gram matvec of the same operator on
                  64 vectors (mfx_op_apply): the kernel generates n m feature entries where the matvec generates n^2 kernel entries
  paths(xs)       a whole evaluation of the S posterior functions at 10^5 test points (one evaluate, one cross_apply, the mean), and
                  the same with the gradient onto the points; the construction (one batched solve) is timed once and reported
                  apart
  covariance      the dense route to draws at the same problem: RbfGramOp.posterior_covariance + gp_util.posterior_samples at
                  --dense-points test points (O(points^2) memory, one solve per 64 points), against paths(xs) at those points;
                  it does not depend on m and is timed once

Every solve is cg.cg_adaptive(atol=--atol, rtol=0, maxiter=--maxiter, miniter=1): the dense route needs converged solves, or the
covariance it factors is indefinite; the step counts are reported.

One window is --inner back-to-back calls between two hipEvents, reported as median [min, max] ms over --reps windows after one untimed
call.  One JSON line per m on stdout.

  python tools/bench_pathwise.py [--n 131072] [--test-points 100000] [--dense-points 1024] [--reps 5] [--inner 3] [--atol 1e-4]
                                  [--maxiter 300] [--jitter 1e-2]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
import torch  # noqa: E402
from matfree_extensions import cg  # noqa: E402
from matfree_extensions.operators import RandomFeatures  # noqa: E402
from matfree_extensions.util import gp_util  # noqa: E402


def timed_ms(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def windows(fn, reps, inner):
    timed_ms(fn, 1)
    v = [timed_ms(fn, inner) for _ in range(reps)]
    return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--features", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--test-points", type=int, default=100000)
    ap.add_argument("--dense-points", type=int, default=1024)
    ap.add_argument("--atol", type=float, default=1e-4)
    ap.add_argument("--maxiter", type=int, default=300)
    ap.add_argument("--jitter", type=float, default=1e-2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    n, d, S = args.n, args.d, args.samples
    X = torch.randn(n, d, device=dev, generator=gen)
    y = torch.sin(X.sum(1)) + 0.1 * torch.randn(n, device=dev, generator=gen)
    xs = torch.randn(args.test_points, d, device=dev, generator=gen)
    xd = xs[: args.dense_points].contiguous()
    raw = [torch.tensor(v, device=dev) for v in (0.5, 0.5, -2.0)]
    op = gp_util.gram_operator(X, noise_minval=1e-4)
    bound = op.bind(*raw)
    ls, s, _ = op.constrain(*raw)
    solve = cg.cg_adaptive(atol=args.atol, rtol=0.0, maxiter=args.maxiter, miniter=1)
    mean = lambda _x: torch.zeros((), device=dev)  # noqa: E731
    mean.batched = lambda pts: torch.zeros(pts.shape[0], device=dev)
    V = torch.randn(S, n, device=dev, generator=gen)

    def dense_draws():
        cov = op.posterior_covariance(xd, solve, *raw)
        return gp_util.posterior_samples(3, torch.zeros(xd.shape[0], device=dev), cov, num=S, jitter=args.jitter)

    with torch.no_grad():
        _, cinfo = op.posterior_covariance(xd, solve, *raw, return_info=True)
        dense_steps = int(cinfo["solve"]["num_steps"].max())
        try:
            dense = windows(dense_draws, max(1, args.reps // 2), 1)
        except ValueError as err:  # the covariance stayed indefinite beyond the jitter
            dense = f"failed: {err}"
    for m in args.features:
        feats = RandomFeatures(1, kernel="rbf", dim=d, num_features=m, num_samples=S, like=X)
        out = {"n": n, "d": d, "samples": S, "features": m, "dtype": "float32", "unit": "ms: median [min, max]"}
        with torch.no_grad():
            out["evaluate"] = windows(lambda: feats.evaluate(X, ls, s), args.reps, args.inner)
            out["gram_matvec"] = windows(lambda: bound(V), args.reps, args.inner)
            out["construct_paths_once"] = round(timed_ms(lambda: gp_util.PathwisePosterior(bound, solve, mean, feats, X, y, key=2), 1), 3)
            paths = gp_util.PathwisePosterior(bound, solve, mean, feats, X, y, key=2)
            out["paths_at_test_points"] = windows(lambda: paths(xs), args.reps, args.inner)
            out["paths_at_dense_points"] = windows(lambda: paths(xd), args.reps, args.inner)

        def with_grad():
            pts = xs.clone().requires_grad_()
            paths(pts).sum().backward()

        out["paths_and_gradient_at_test_points"] = windows(with_grad, args.reps, args.inner)
        out["covariance_and_samples_at_dense_points"], out["covariance_solve_max_steps"] = dense, dense_steps
        out["paths_solve_max_steps"] = int(paths.info["solve"]["num_steps"].max())
        out["test_points"], out["dense_points"] = args.test_points, args.dense_points
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
