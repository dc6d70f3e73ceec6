"""The GP predictive variance (RbfGramOp.posterior_variance), fp32, over the shapes of DESIGN.md section 3.3d: the forward split
into its three parts (B = K(xs, X) by mfx_gram_cross_apply_t against the identity, the batched solve, the row-wise <B, W>) and the
backward without the X gradient split into its parts (the dense cross sweep for xs, l, s; the Gram parameter sweep
mfx_op_vjp_params for l, s, noise), then the dense sweep against the factored mfx_gram_cross_vjp with L = I (batch = m) at
m = 64 and 1024.  The solver is cg_fixed_step(--cg-steps): a fixed cost, so that forward times are comparable between runs; the
backward does not depend on it.  Times are medians of --reps runs, each bracketed by synchronisations.

  python tools/bench_posterior_var.py [--reps R] [--cg-steps K] [--chunk C]

One JSON line per measurement on stdout.  The log of a run on the MI355X is kept under profiles/."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "experiments-lanczos-adjoints_amd"))
import torch  # noqa: E402
from matfree_extensions import _lib, cg  # noqa: E402
from matfree_extensions.operators import RbfGramOp  # noqa: E402

SHAPES = [(1024, 131072, 8, "rbf", True), (256, 45730, 9, "matern32", True), (256, 100000, 90, "rbf", True)]
SWEEP_SHAPES = [(64, 131072, 8), (1024, 131072, 8)]


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


def problem(m, n, d, ard, dev, seed=7):
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn((n, d), generator=g) / math.sqrt(d / 8)).to(dev)
    xs = (torch.randn((m, d), generator=g) / math.sqrt(d / 8)).to(dev)
    vbar = torch.randn((m,), generator=g).to(dev)
    raw = [torch.tensor(r, dtype=torch.float32, device=dev)
           for r in ([inv_softplus(1.5)] * d if ard else inv_softplus(1.5), inv_softplus(1.0), inv_softplus(0.1))]
    return X, xs, vbar, raw


def bench_variance(m, n, d, kind, ard, args, dev):
    X, xs, vbar, raw = problem(m, n, d, ard, dev)
    op = RbfGramOp(X, kernel=kind)
    solve = cg.cg_fixed_step(args.cg_steps)
    bound = op.bind(*raw)
    cparams = op.constrain(*raw)
    desc = op.descriptor(cparams, torch.float32, n)
    lib, stream = _lib.get(), _lib.stream_ptr(dev)
    chunks = [(a0, min(args.chunk, m - a0)) for a0 in range(0, m, args.chunk)]
    Bs = [torch.empty((c, n), device=dev) for _, c in chunks]

    def part_b():
        for (a0, c), B in zip(chunks, Bs):
            eye = torch.eye(c, device=dev)
            ws = _lib.scratch(int(lib.mfx_gram_cross_workspace_bytes(C.byref(desc), c)), dev)
            _lib.check(lib.mfx_gram_cross_apply_t(C.byref(desc), _lib.ptr(xs[a0:a0 + c]), c, _lib.ptr(eye), c, _lib.ptr(B), n, c,
                                                  _lib.ptr(ws), ws.numel(), stream))

    part_b()
    Ws = []

    def part_solve():
        Ws.clear()
        with torch.no_grad():
            for B in Bs:
                Ws.append(solve(bound, B)[0])

    part_solve()

    def part_q():
        for B, W in zip(Bs, Ws):
            (B * W).sum(-1)

    W = torch.cat(Ws)
    S = torch.empty_like(W)

    def part_sweep():  # the dense cross sweep for xs, l, s, as the backward calls it
        torch.mul(W, (-2.0 * vbar)[:, None], out=S)
        gl, gs, gxs = torch.zeros_like(cparams[0]), torch.zeros_like(cparams[1]), torch.zeros_like(xs)
        st = _lib.OpGrads()
        st.lengthscale, st.outputscale = gl.data_ptr(), gs.data_ptr()
        ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_dense_workspace_bytes(C.byref(desc), m)), dev)
        _lib.check(lib.mfx_gram_cross_vjp_dense(C.byref(desc), _lib.ptr(xs), m, _lib.ptr(S), n, C.byref(st), _lib.ptr(gxs),
                                                _lib.ptr(ws), ws.numel(), stream))

    def part_params():  # the Gram parameter sweep for l, s, noise with L = vbar W, R = W
        L = W * vbar[:, None]
        g = [torch.zeros_like(t) for t in cparams[:3]]
        st = _lib.OpGrads()
        st.lengthscale, st.outputscale, st.noise = (t.data_ptr() for t in g)
        ws = _lib.workspace(desc, n, 1, m, dev)
        _lib.check(lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(L), n, _lib.ptr(W), n, m, C.byref(st), _lib.ptr(ws), ws.numel(),
                                         stream))

    def forward():
        with torch.no_grad():
            op.posterior_variance(xs, solve, *raw, chunk=args.chunk)

    def fwd_bwd():
        xg = xs.clone().requires_grad_(True)
        params = [r.clone().requires_grad_(True) for r in raw]
        var = op.posterior_variance(xg, solve, *params, chunk=args.chunk)
        torch.autograd.grad((vbar * var).sum(), [xg, *params])

    t = {k: median_ms(f, args.reps) for k, f in (("fwd_B_ms", part_b), ("fwd_solve_ms", part_solve), ("fwd_q_ms", part_q),
                                                  ("bwd_cross_sweep_ms", part_sweep), ("bwd_param_sweep_ms", part_params))}
    t_fwd = median_ms(forward, args.reps)
    t_all = median_ms(fwd_bwd, args.reps)
    out = {"m": m, "n": n, "d": d, "dtype": "fp32", "kernel": kind, "ard": ard, "chunk": args.chunk, "cg_steps": args.cg_steps,
           **{k: round(v, 3) for k, v in t.items()}, "forward_ms": round(t_fwd, 3), "fwd_bwd_no_X_ms": round(t_all, 3),
           "bwd_no_X_over_fwd": round((t_all - t_fwd) / t_fwd, 3)}
    print(json.dumps(out), flush=True)


def bench_sweep(m, n, d, args, dev):
    X, xs, vbar, raw = problem(m, n, d, True, dev, seed=11)
    op = RbfGramOp(X)
    cparams = op.constrain(*raw)
    desc = op.descriptor(cparams, torch.float32, n)
    lib, stream = _lib.get(), _lib.stream_ptr(dev)
    S = torch.randn((m, n), device=dev)
    eye = torch.eye(m, device=dev)
    res = {}

    def run(dense, want_x):
        g = [torch.zeros_like(cparams[0]), torch.zeros_like(cparams[1]), torch.zeros_like(xs), torch.zeros_like(X)]
        st = _lib.OpGrads()
        st.lengthscale, st.outputscale = g[0].data_ptr(), g[1].data_ptr()
        if want_x:
            st.x = g[3].data_ptr()
        if dense:
            ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_dense_workspace_bytes(C.byref(desc), m)), dev)
            _lib.check(lib.mfx_gram_cross_vjp_dense(C.byref(desc), _lib.ptr(xs), m, _lib.ptr(S), n, C.byref(st), _lib.ptr(g[2]),
                                                    _lib.ptr(ws), ws.numel(), stream))
        else:
            ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_workspace_bytes(C.byref(desc), m, m)), dev)
            _lib.check(lib.mfx_gram_cross_vjp(C.byref(desc), _lib.ptr(xs), m, _lib.ptr(eye), m, _lib.ptr(S), n, m, C.byref(st),
                                              _lib.ptr(g[2]), _lib.ptr(ws), ws.numel(), stream))
        return g

    for want_x in (False, True):
        tag = "with_X" if want_x else "no_X"
        res[f"dense_{tag}_ms"] = round(median_ms(lambda: run(True, want_x), args.reps), 3)
        res[f"factored_diag_L_{tag}_ms"] = round(median_ms(lambda: run(False, want_x), args.reps), 3)
    a, b = run(True, True), run(False, True)
    torch.cuda.synchronize()
    err = max(float((x - y).abs().max()) / max(float(y.abs().max()), 1e-30) for x, y in zip(a, b))
    print(json.dumps({"sweep": "dense vs factored (L = I, batch = m)", "m": m, "n": n, "d": d, "dtype": "fp32", "kernel": "rbf",
                      "ard": True, **res, "speedup_no_X": round(res["factored_diag_L_no_X_ms"] / res["dense_no_X_ms"], 2),
                      "speedup_with_X": round(res["factored_diag_L_with_X_ms"] / res["dense_with_X_ms"], 2),
                      "max_rel_diff": err}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cg-steps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--only", choices=["variance", "sweep", "all"], default="all")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.only in ("sweep", "all"):
        for m, n, d in SWEEP_SHAPES:
            bench_sweep(m, n, d, args, dev)
    if args.only in ("variance", "all"):
        for shape in SHAPES:
            bench_variance(*shape, args, dev)


if __name__ == "__main__":
    main()
