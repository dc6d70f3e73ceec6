"""The config-4 SLQ step (n = 131072, d = 8, k = 40, 64 probes, fp32, RBF) with and without the gradient with respect to the
inputs X: step times, the input sweep's time as the delta of the parameter-sweep timing class (class 1), and the accuracy of
dG/dX in each fp32 mode against the fp64 path on the same probes (relative Frobenius error, worst row).  --sweep-batch B: the input
sweep alone (mfx_op_vjp_params with only `x`) in fp32 against fp64 on the SAME L, R (random, B rows): the sweep's own arithmetic,
apart from the fp32 Krylov states that feed it in a step.

  python tools/bench_input_grad.py [--n N] [--d D] [--k K] [--probes P] [--steps S] [--no-fp64] [--no-step] [--sweep-batch B]

One JSON line per measurement on stdout.  The log of a run on the MI355X is kept under profiles/."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "experiments-lanczos-adjoints_amd"))
import torch  # noqa: E402
from matfree_extensions import _lib, hutchinson, lanczos  # noqa: E402
from matfree_extensions.util import gp_util  # noqa: E402


def inv_softplus(v):
    return math.log(math.expm1(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--no-fp64", action="store_true", help="skip the fp64 reference (and so the accuracy lines)")
    ap.add_argument("--no-step", action="store_true", help="skip the step timings and their accuracy")
    ap.add_argument("--sweep-batch", type=int, default=0, help="> 0: also the sweep-only accuracy with this many L, R rows")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d, k = args.n, args.d, args.k
    gen = torch.Generator().manual_seed(4)
    X0 = torch.randn((n, d), generator=gen, dtype=torch.float32).to(dev)  # bench.py's inputs
    sampler = hutchinson.sampler_rademacher(X0[:, 0], num=args.probes)

    def step(dtype, precision, x_grad, seed=0):
        params = [torch.tensor(v, dtype=dtype, device=dev, requires_grad=True) for v in (inv_softplus(2.0), inv_softplus(1.0),
                                                                                         inv_softplus(0.1))]
        X = X0.to(dtype).requires_grad_(x_grad)
        integrand = lanczos.integrand_spd(torch.log, k, gp_util.gram_operator(X, precision=precision))
        values = integrand(sampler((seed, 0)).to(dtype), *params)
        grads = torch.autograd.grad(values.sum(), params + ([X] if x_grad else []))
        return grads

    def timed(dtype, precision, x_grad, steps):
        step(dtype, precision, x_grad, seed=100)  # warm-up
        torch.cuda.synchronize()
        _lib.timing_reset()
        _lib.timing_enable(True)
        t0 = time.perf_counter()
        for s in range(steps):
            out = step(dtype, precision, x_grad, seed=s)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / steps
        cls = [_lib.timing_read(c)[0] / steps for c in range(3)]
        _lib.timing_enable(False)
        return out, wall, cls

    if args.sweep_batch > 0:
        sweep_only(X0, args.sweep_batch, dev)
    if args.no_step:
        return
    res = {}
    for x_grad in (False, True):
        _, wall, cls = timed(torch.float32, "f16x3", x_grad, args.steps)
        res[x_grad] = (wall, cls)
        print(json.dumps({"what": "step", "x_grad": x_grad, "precision": "f16x3", "n": n, "d": d, "k": k, "probes": args.probes,
                          "seconds_per_step_wall_timed": wall, "class_ms_per_step": {"apply": cls[0], "param_sweep": cls[1],
                                                                                      "krylov_vectors": cls[2]}}), flush=True)
    print(json.dumps({"what": "x_sweep", "ms_per_step_class1_delta": res[True][1][1] - res[False][1][1],
                      "step_ratio_wall_timed": res[True][0] / res[False][0],
                      "note": "both steps run with kernel timing on (events around every class scope)"}), flush=True)
    if args.no_fp64:
        return
    ref = step(torch.float64, "f16x3", True, seed=0)[-1]
    for precision in ("f16x3", "f16x3-matvec", "fp32"):
        gx = step(torch.float32, precision, True, seed=0)[-1].double()
        rows = (gx - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)
        print(json.dumps({"what": "accuracy_vs_fp64", "precision": precision, "n": n,
                          "rel_frobenius": float((gx - ref).norm() / ref.norm()), "worst_row_rel": float(rows.max()),
                          "median_row_rel": float(rows.median())}), flush=True)


def sweep_only(X0, batch, dev):
    import ctypes as C

    from matfree_extensions.operators import RbfGramOp

    n = X0.shape[0]
    gen = torch.Generator(device=dev).manual_seed(1)
    L = torch.randn((batch, n), generator=gen, device=dev, dtype=torch.float64)
    R = torch.randn((batch, n), generator=gen, device=dev, dtype=torch.float64)
    lib, out = _lib.get(), {}
    for dtype in (torch.float64, torch.float32):
        op = RbfGramOp(X0.to(dtype))
        cparams = op.constrain(*(torch.tensor(v, dtype=dtype, device=dev) for v in (inv_softplus(2.0), inv_softplus(1.0),
                                                                                       inv_softplus(0.1))))
        desc = op.descriptor(cparams, dtype, n)
        gx = torch.zeros_like(X0, dtype=dtype)
        st = _lib.OpGrads()
        st.x = gx.data_ptr()
        Lt, Rt = L.to(dtype), R.to(dtype)
        ws = _lib.workspace(desc, n, 1, batch, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(Lt), n, _lib.ptr(Rt), n, batch, C.byref(st), _lib.ptr(ws), ws.numel(),
                                         _lib.stream_ptr(dev)))
        torch.cuda.synchronize()
        out[dtype] = (gx.double(), time.perf_counter() - t0)
    ref, got = out[torch.float64][0], out[torch.float32][0]
    rows = (got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)
    print(json.dumps({"what": "sweep_only_accuracy_vs_fp64", "n": n, "batch": batch, "rel_frobenius": float((got - ref).norm() / ref.norm()),
                      "worst_row_rel": float(rows.max()), "median_row_rel": float(rows.median()),
                      "seconds_fp32": out[torch.float32][1], "seconds_fp64": out[torch.float64][1]}), flush=True)


if __name__ == "__main__":
    main()
