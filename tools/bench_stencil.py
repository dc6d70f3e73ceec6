"""The matrix-free stencil operator (operators.StencilOp) against the assembled CSR form of the same wave system
(pde_util.wave_operator -> CsrOp) at BASELINE config 5's size: res x res grid, state 2 res^2, 5-point Laplacian, Neumann, p = 1.

  apply / transposed apply   mfx_op_apply on both operators; bytes of the stencil form = 5 arrays of res^2 elements (reads u, du and
                             the field, writes two blocks); of the CSR form = val + col (6 res^2 x (elem + 4)) + crow + the vectors
  field gradient, batch 30   StencilOp: one k_stencil_grad sweep onto the field.  CsrOp: k_csr_grad onto the 6 res^2 stored values,
                             then values_fn's backward (the segment sum onto the field)
  end to end                 pde_util.expm_arnoldi(k = 30): forward, and forward + backward of <w, exp(dt A) y0> with respect to the
                             field -- the CSR operator takes the fused step head inside the driver (k_csr_step), the stencil does not

Both operators in one process on the same data, timed in alternation (A B A B ...): one window is --inner back-to-back calls between
two hipEvents (end to end: one call, ended by a synchronise), reported as median [min, max] over --reps windows after one untimed round.
Before timing, the two operators' results are compared at the timed size.  One JSON line per dtype on stdout.

  python tools/bench_stencil.py [--res 1000] [--reps 7] [--inner 20]"""
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
from matfree_extensions.operators import StencilOp  # noqa: E402
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
    return {name: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for name, v in samples.items()}


def raw_apply(op, cparams, x, y, transpose):
    lib, n = _lib.get(), x.numel()
    desc = op.descriptor(cparams, x.dtype, n)
    ws = _lib.workspace(desc, n, 1, 1, x.device)
    args = (C.byref(desc), _lib.ptr(x), n, _lib.ptr(y), n, 1, int(transpose), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device))
    return lambda: _lib.check(lib.mfx_op_apply(*args)), desc  # desc is kept alive by the caller


def raw_grad(op, cparams, L, R, g):
    lib, n = _lib.get(), L.shape[1]
    desc = op.descriptor(cparams, L.dtype, n)
    st = _lib.OpGrads()
    st.val = g.data_ptr()
    ws = _lib.workspace(desc, n, 1, L.shape[0], L.device)
    args = (C.byref(desc), _lib.ptr(L), n, _lib.ptr(R), n, L.shape[0], C.byref(st), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(L.device))
    return lambda: _lib.check(lib.mfx_op_vjp_params(*args)), (desc, st)


def relerr(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--dtypes", default="float64,float32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stencil needs a GPU"
    dev = torch.device("cuda:0")
    res, m = args.res, args.res * args.res
    n = 2 * m
    for dtname in args.dtypes.split(","):
        dt = getattr(torch, dtname)
        es = torch.empty((), dtype=dt).element_size()
        gen = torch.Generator(device=dev).manual_seed(0)
        scale = ((0.01 * torch.randn((res, res), dtype=dt, device=dev, generator=gen)) ** 2 + 1e-6)
        x = torch.randn(n, dtype=dt, device=dev, generator=gen)
        csr, values_fn = pde_util.wave_operator(res, 1.0 / res, boundary="neumann", device=dev, dtype=dt)
        sop = StencilOp(res, pde_util.stencil_laplacian(1.0 / res), form="wave", boundary="neumann")
        vals = values_fn(scale).detach()
        coef = scale.reshape(-1).contiguous()
        ys, yc = torch.empty_like(x), torch.empty_like(x)
        out = {"tool": "bench_stencil", "res": res, "dtype": dtname, "n": n, "nnz": csr.nnz}
        keep = []
        bytes_stencil = 5 * m * es
        bytes_csr = csr.nnz * (es + 4) + (n + 1) * 4 + 2 * n * es
        for transpose in (0, 1):
            fs, d1 = raw_apply(sop, (coef,), x, ys, transpose)
            fc, d2 = raw_apply(csr, (vals,), x, yc, transpose)
            keep += [d1, d2]
            fs(), fc()
            key = "apply_t" if transpose else "apply"
            out[key + "_relerr_vs_csr"] = relerr(ys, yc)
            t = alternate({"stencil": fs, "csr": fc}, args.reps, args.inner)
            out[key + "_ms"] = t
            out[key + "_GBps"] = {"stencil": round(bytes_stencil / t["stencil"][0] / 1e6, 1), "csr": round(bytes_csr / t["csr"][0] / 1e6, 1)}
        out["bytes_model"] = {"stencil": bytes_stencil, "csr": bytes_csr}
        # field gradient at batch 30
        L = torch.randn((args.batch, n), dtype=dt, device=dev, generator=gen)
        R = torch.randn((args.batch, n), dtype=dt, device=dev, generator=gen)
        gs, gv = torch.zeros(m, dtype=dt, device=dev), torch.zeros(csr.nnz, dtype=dt, device=dev)
        fgs, k1 = raw_grad(sop, (coef,), L, R, gs)
        fgc_sweep, k2 = raw_grad(csr, (vals,), L, R, gv)
        keep += [k1, k2]
        sreq = scale.clone().requires_grad_(True)
        vreq = values_fn(sreq)

        def fgc():
            fgc_sweep()
            return torch.autograd.grad(vreq, sreq, gv, retain_graph=True)[0]

        fgs()
        ref = fgc().reshape(-1)
        out["grad_relerr_vs_csr"] = relerr(gs, ref)
        out["grad_ms"] = alternate({"stencil": fgs, "csr_sweep_plus_values_bwd": fgc}, args.reps, max(1, args.inner // 4))
        del L, R, gv, vreq
        # end to end: expm_arnoldi, forward and forward + backward
        expm = pde_util.expm_arnoldi(args.depth)
        w = torch.randn(n, dtype=dt, device=dev, generator=gen)
        dtm = 1e-3

        def fwd_s():
            with torch.no_grad():
                return expm(sop, dtm, x, coef)[0]

        def fwd_c():
            with torch.no_grad():
                return expm(csr, dtm, x, vals)[0]

        def fb_s():
            s = scale.clone().requires_grad_(True)
            return torch.autograd.grad((expm(sop, dtm, x, s)[0] * w).sum(), s)[0]

        def fb_c():
            s = scale.clone().requires_grad_(True)
            return torch.autograd.grad((expm(csr, dtm, x, values_fn(s))[0] * w).sum(), s)[0]

        out["expm_relerr_vs_csr"] = relerr(fwd_s(), fwd_c())
        out["expm_grad_relerr_vs_csr"] = relerr(fb_s(), fb_c())
        out["expm_forward_ms"] = alternate({"stencil": fwd_s, "csr": fwd_c}, args.reps, 2)
        out["expm_forward_backward_ms"] = alternate({"stencil": fb_s, "csr": fb_c}, args.reps, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
