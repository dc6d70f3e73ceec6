"""The fixed-step Runge-Kutta baselines (pde_util.solver_rk -> mfx_rk_solve / mfx_rk_adjoint / mfx_rk_backsolve) at BASELINE config 5's
shape: res x res grid, wave form, Neumann, state 2 res^2, p = 1, fp64 and fp32, on the matrix-free stencil operator.

  methods      each tableau at the reference's step counts (workprecision.py: 1 .. num_steps_max - 1), forward and forward + backward of
               <w, y(1)> with respect to the field, for both adjoints
  expm         pde_util.expm_arnoldi(k = 30) in the same process, forward and forward + backward

The fused stencil stage kernel was measured with an earlier form of this tool (entry "fuse_dopri5_ms" of profiles/r18a_bench_rk.log) and
did not ship: tools/experiments/rk_fused_stage, DESIGN.md section 3.4b.

One window is --inner back-to-back calls between two hipEvents, ended by a synchronise; median [min, max] over --reps windows after
one untimed round.  Timing only: at dx = 1 / res the explicit methods are far outside their stability region, which the kernels
do not care about (the field is scaled down so that nothing overflows).  One JSON line per dtype on stdout.

  python tools/bench_rk.py [--res 1000] [--reps 7] [--inner 3] [--steps 1,3,9]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
import torch  # noqa: E402
from matfree_extensions import _lib  # noqa: E402
from matfree_extensions.operators import StencilOp  # noqa: E402
from matfree_extensions.util import pde_util, rk_tableaux  # noqa: E402


def timed_ms(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def alternate(fns, reps, inner):
    """{name: [median, min, max] ms per call}; the candidates take turns window by window"""
    for fn in fns.values():
        timed_ms(fn, 1)
    samples = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            samples[name].append(timed_ms(fn, inner))
    return {name: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--steps", default="1,2,3,4,5,6,7,8,9")
    ap.add_argument("--methods", default="euler,heun,rk4,dopri5,dopri8")
    ap.add_argument("--dtypes", default="float64,float32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rk needs a GPU"
    dev = torch.device("cuda:0")
    res, m = args.res, args.res * args.res
    n = 2 * m
    steps = [int(s) for s in args.steps.split(",")]
    for dtname in args.dtypes.split(","):
        dt = getattr(torch, dtname)
        gen = torch.Generator(device=dev).manual_seed(0)
        scale = ((1e-3 * torch.randn((res, res), dtype=dt, device=dev, generator=gen)) ** 2 + 1e-9) / res**2
        y0 = torch.randn(n, dtype=dt, device=dev, generator=gen)
        w = torch.randn(n, dtype=dt, device=dev, generator=gen)
        sop = StencilOp(res, pde_util.stencil_laplacian(1.0 / res), form="wave", boundary="neumann")
        out = {"tool": "bench_rk", "res": res, "dtype": dtname, "n": n, "reps": args.reps, "inner": args.inner}

        def forward(solver):
            def run():
                with torch.no_grad():
                    return solver(y0, scale)[0]

            return run

        def forward_backward(solver):
            def run():
                s = scale.clone().requires_grad_(True)
                return torch.autograd.grad((solver(y0, s)[0] * w).sum(), s)[0]

            return run

        table = {}
        for method in args.methods.split(","):
            stages = len(rk_tableaux.get(method).b)
            for ns in steps:
                fns = {}
                for adjoint in ("discrete", "backsolve"):
                    solver = pde_util.solver_rk(0.0, 1e-3, sop, num_steps=ns, method=method, adjoint=adjoint)
                    if adjoint == "discrete":
                        fns["forward"] = forward(solver)
                    fns[f"fwd_bwd_{adjoint}"] = forward_backward(solver)
                table[f"{method}:{ns}"] = {"applies": ns * stages, **alternate(fns, args.reps, args.inner)}
        out["rk_ms"] = table
        expm = pde_util.solver_expm(0.0, 1e-3, sop, expm=pde_util.expm_arnoldi(args.depth))
        out[f"expm_arnoldi_k{args.depth}_ms"] = alternate({"forward": forward(expm), "fwd_bwd": forward_backward(expm)}, args.reps, args.inner)
        out["graphs"] = dict(zip(("captured", "replayed"), _lib.graph_stats()))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
