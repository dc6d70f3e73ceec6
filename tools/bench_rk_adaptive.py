"""The adaptive-step Runge-Kutta solve (pde_util.solver_rk_adaptive -> mfx_rk_solve_adaptive) at BASELINE config 5's shape: res x res
grid, wave form, Neumann, state 2 res^2, p = 1, dopri5, on the matrix-free stencil operator with a smooth coefficient field
(0.3 + 0.05 sin sin)^2 and a Gaussian bump as the initial state, t in [0, --t1].

  per attempt   the adaptive forward solve, ms per attempt (accepted + rejected), against mfx_rk_solve with the accepted step sizes,
                ms per step: what the error pass, the controller, the commit and the chunked polling cost on top of a step
  chunks        --chunks (default 1, 8, 32): attempts enqueued between two reads of the control block
  tail          the share of launched attempts that ran after the solve was over: (chunks x chunk - attempts) / (chunks x chunk)

One window is --inner back-to-back calls between two hipEvents, ended by a synchronise; median [min, max] over --reps windows after
one untimed round, the candidates taking turns.  One JSON line per dtype on stdout.

  python tools/bench_rk_adaptive.py [--res 1000] [--reps 7] [--inner 2] [--rtol 1e-4] [--t1 0.02]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from bench_rk import alternate  # noqa: E402
from matfree_extensions import _lib  # noqa: E402
from matfree_extensions.operators import StencilOp  # noqa: E402
from matfree_extensions.util import pde_util  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--rtol", type=float, default=1e-4)
    ap.add_argument("--t1", type=float, default=0.02)
    ap.add_argument("--chunks", default="1,8,32")
    ap.add_argument("--dtypes", default="float64,float32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rk_adaptive needs a GPU"
    dev = torch.device("cuda:0")
    res = args.res
    n = 2 * res * res
    for dtname in args.dtypes.split(","):
        dt = getattr(torch, dtname)
        xs = torch.linspace(0.0, 1.0, res, dtype=dt, device=dev)
        field = (0.3 + 0.05 * torch.sin(6.0 * xs)[:, None] * torch.sin(4.0 * xs)[None, :]) ** 2
        bump = torch.exp(-40.0 * ((xs[:, None] - 0.5) ** 2 + (xs[None, :] - 0.4) ** 2))
        y0 = torch.cat([bump.reshape(-1), torch.zeros_like(bump).reshape(-1)])
        sop = StencilOp(res, pde_util.stencil_laplacian(1.0 / (res - 1)), form="wave", boundary="neumann")
        solver = pde_util.solver_rk_adaptive(0.0, args.t1, sop, method="dopri5", rtol=args.rtol, atol=1e-3 * args.rtol)
        with torch.no_grad():
            y1, info = solver(y0, field)
        attempts = info["num_steps"] + info["num_rejected"]
        out = {"tool": "bench_rk_adaptive", "res": res, "dtype": dtname, "n": n, "reps": args.reps, "inner": args.inner, "rtol": args.rtol,
               "t1": args.t1, "num_steps": info["num_steps"], "num_rejected": info["num_rejected"], "dt_min": min(info["dts"]),
               "dt_max": max(info["dts"]), "max_abs_y1": float(y1.abs().max())}
        fixed = pde_util._rk_solver(info["dts"], sop, "dopri5", "discrete")
        fns = {"fixed_same_dts": lambda: torch.no_grad()(lambda: fixed(y0, field)[0])()}
        chunks = [int(c) for c in args.chunks.split(",")]
        for chunk in chunks:
            fns[f"adaptive_chunk{chunk}"] = (lambda c: lambda: torch.no_grad()(lambda: solver(y0, field, chunk=c)[0])())(chunk)
        ms = alternate(fns, args.reps, args.inner)
        out["solve_ms"] = ms
        out["fixed_ms_per_step"] = round(ms["fixed_same_dts"][0] / info["num_steps"], 4)
        for chunk in chunks:
            launched = math.ceil(attempts / chunk) * chunk
            out[f"chunk{chunk}"] = {"ms_per_attempt": round(ms[f"adaptive_chunk{chunk}"][0] / attempts, 4), "host_syncs": launched // chunk,
                                    "tail_share": round((launched - attempts) / launched, 4)}
        out["graphs"] = dict(zip(("captured", "replayed"), _lib.graph_stats()))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
