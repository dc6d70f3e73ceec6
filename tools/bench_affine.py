"""The bordered affine operator (operators.AffineOp around a StencilOp) against the bare StencilOp at BASELINE config 5's grid:
res x res cells, heat form, 5-point Laplacian, Neumann, p = 1 and 8.

  apply / transposed apply   mfx_op_apply on both.  The border adds, per probe, one read of b and one read-modify-write of y
                             (k_affine_border: 3 passes over an n-vector) or one read of b and of x (k_affine_dot: 2 passes)
  drift + field gradient     mfx_op_vjp_params, batch = 8 p: the stencil's own sweep, plus k_affine_grad_b (batch + 2 passes)
  solver_rk dopri5, 9 steps  forward, and forward + backward (discrete adjoint) with gradients onto y0 and the parameters
  expm_arnoldi, k = 30       forward, and forward + backward

Both operators in one process on the same data, timed in alternation (A B A B ...): one window is --inner back-to-back calls
between two hipEvents (end to end: one call, ended by a synchronise), reported as median [min, max] over --reps windows after one
untimed round, with the ratio of the medians.  One JSON line per (dtype, p) on stdout.

  python tools/bench_affine.py [--res 1000] [--reps 7] [--inner 20] [--dtypes f64]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
import torch  # noqa: E402
from matfree_extensions import _lib  # noqa: E402
from matfree_extensions.operators import AffineOp, StencilOp  # noqa: E402
from matfree_extensions.util import pde_util  # noqa: E402


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
    out = {name: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for name, v in samples.items()}
    out["ratio"] = round(out["affine"][0] / out["stencil"][0], 3)
    return out


def raw_apply(op, cparams, X, transpose):
    lib = _lib.get()
    p, n = X.shape
    desc = op.descriptor(cparams, X.dtype, n)
    ws = _lib.workspace(desc, n, 1, p, X.device)
    Y = torch.empty_like(X)
    args = (C.byref(desc), _lib.ptr(X), n, _lib.ptr(Y), n, p, int(transpose), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(X.device))
    return lambda: _lib.check(lib.mfx_op_apply(*args)), (desc, Y, ws)


def raw_grad(op, cparams, L, R):
    lib = _lib.get()
    batch, n = L.shape
    desc = op.descriptor(cparams, L.dtype, n)
    st, grads = op.new_grads(*cparams)
    ws = _lib.workspace(desc, n, 1, batch, L.device)
    args = (C.byref(desc), _lib.ptr(L), n, _lib.ptr(R), n, batch, C.byref(st), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(L.device))
    return lambda: _lib.check(lib.mfx_op_vjp_params(*args)), (desc, st, grads, ws)


def end_to_end(solve, y0, params, w, backward):
    def run():
        leaves = [t.detach().requires_grad_(backward) for t in (y0, *params)]
        y1, _ = solve(leaves[0], *leaves[1:])
        if backward:
            torch.autograd.grad(y1, leaves, w)
        torch.cuda.synchronize()

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--dtypes", default="f64")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = args.res
    m = res * res
    dx = 1.0 / res
    for name in args.dtypes.split(","):
        dtype = {"f64": torch.float64, "f32": torch.float32}[name]
        gen = torch.Generator(device=dev).manual_seed(0)
        rnd = lambda *shape: torch.randn(shape, dtype=dtype, device=dev, generator=gen)  # noqa: E731
        stencil = StencilOp((res, res), pde_util.stencil_laplacian(dx), form="heat", boundary="neumann")
        affine = AffineOp(stencil)
        coef = 0.5 + torch.rand((res, res), dtype=dtype, device=dev, generator=gen)
        drift = rnd(m)
        ps, pa = stencil.constrain(coef), affine.constrain(coef, drift)
        for p in (1, 8):
            out = {"dtype": name, "res": res, "p": p}
            keep = []
            for what, transpose in (("apply", False), ("apply_t", True)):
                fs, k1 = raw_apply(stencil, ps, rnd(p, m), transpose)
                fa, k2 = raw_apply(affine, pa, rnd(p, m + 1), transpose)
                keep += [k1, k2]
                out[what] = alternate({"stencil": fs, "affine": fa}, args.reps, args.inner)
            batch = 8 * p
            fs, k1 = raw_grad(stencil, ps, rnd(batch, m), rnd(batch, m))
            fa, k2 = raw_grad(affine, pa, rnd(batch, m + 1), rnd(batch, m + 1))
            out["vjp_batch"] = batch
            out["vjp"] = alternate({"stencil": fs, "affine": fa}, args.reps, max(1, args.inner // 4))
            y0, w = rnd(p, m), rnd(p, m)
            dt = 0.1 * dx * dx  # dt |A| ~ 1: stable steps
            for what, make in (("rk_dopri5_9", lambda op: pde_util.solver_rk(0.0, 9 * dt, op, num_steps=9, method="dopri5")),
                               ("expm_arnoldi_30", lambda op: pde_util.solver_expm(0.0, 9 * dt, op, expm=pde_util.expm_arnoldi(30)))):
                if what.startswith("expm") and p > 1:
                    continue  # solver_expm takes one state of a plain operator
                for backward in (False, True):
                    fns = {"stencil": end_to_end(make(stencil), y0 if p > 1 else y0[0], (coef,), w if p > 1 else w[0], backward),
                           "affine": end_to_end(make(affine), y0 if p > 1 else y0[0], (coef, drift), w if p > 1 else w[0], backward)}
                    out[what + ("_fwd_bwd" if backward else "_fwd")] = alternate(fns, args.reps, 1)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
