"""The basis combination of f(A) v (mfx_basis_combine, mfx_basis_combine_bwd) against the torch expressions the package uses for it
today, at the vector shapes of BASELINE configs 5 and 4:

  C5  n = 2 000 000, k = 30, p = 1,  fp64        C4  n = 131 072, k = 40, p = 64, fp32

  native forward    y = sum_j c_j q_j                               reads Q, writes y
  native backward   dQ = c dy^T and dc = Q dy                       reads Q and dy, writes dQ
  torch "weighted"  (Q * c[..., None]).sum(-2)                      pde_util.expm_arnoldi's form, and autograd through it
  torch "einsum"    einsum("bkn,bk->bn", Q, c)                      pde_util.sampler_lanczos' form, and autograd through it

All on random data in one process, timed in alternation (A B C A B C ...): one timed window is --inner back-to-back calls between two
hipEvents on the current stream (a single call is 0.1 - 2 ms: launch overhead and the event resolution would be a visible share of it),
reported per call as median [min, max] over --reps windows after one untimed round.  Achieved bytes per second of the native kernels
count the algorithmic bytes above at the median; --krylov-gbps takes the `roofline.krylov_vector_hbm.achieved_GBps` figure of a
`bench.py --full` line from the same box and reports the ratio.  Before timing, the native y, dQ and dc are compared with the fp64 einsum
forms at the timed size.

  python tools/bench_funm.py [--reps R] [--inner N] [--krylov-gbps G]

One JSON line per shape on stdout."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
import torch  # noqa: E402
from matfree_extensions import _lib  # noqa: E402

SHAPES = {"C5": (2_000_000, 30, 1, torch.float64), "C4": (131_072, 40, 64, torch.float32)}


def timed_ms(fn, inner):
    """milliseconds per call over one window of `inner` back-to-back calls"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def relerr(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--krylov-gbps", type=float, default=0.0)
    ap.add_argument("--shapes", default="C5,C4")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.get()
    for name in args.shapes.split(","):
        n, k, p, dt = SHAPES[name]
        es, code, stream = torch.empty((), dtype=dt).element_size(), _lib.dtype_code(dt), _lib.stream_ptr(dev)
        gen = torch.Generator(device=dev).manual_seed(0)
        Q = torch.randn((p, k, n), dtype=dt, device=dev, generator=gen)
        c = torch.randn((p, k), dtype=dt, device=dev, generator=gen)
        dy = torch.randn((p, n), dtype=dt, device=dev, generator=gen)
        y, dQ, dc = torch.empty_like(dy), torch.empty_like(Q), torch.empty_like(c)
        ws = torch.empty(int(lib.mfx_basis_combine_workspace_bytes(n, k, p, code)), dtype=torch.uint8, device=dev)
        Qg, cg = Q.clone().requires_grad_(True), c.clone().requires_grad_(True)

        def native_fwd():
            _lib.check(lib.mfx_basis_combine(_lib.ptr(Q), _lib.ptr(c), n, k, p, code, _lib.ptr(y), stream))

        def native_bwd():
            _lib.check(lib.mfx_basis_combine_bwd(_lib.ptr(Q), _lib.ptr(c), _lib.ptr(dy), n, k, p, code, _lib.ptr(dQ), _lib.ptr(dc), _lib.ptr(ws),
                                                 ws.numel(), stream))

        forms = {"weighted": lambda Q_, c_: (Q_ * c_[..., None]).sum(dim=-2), "einsum": lambda Q_, c_: torch.einsum("bkn,bk->bn", Q_, c_)}
        legs = {"native_fwd": native_fwd, "native_bwd": native_bwd}
        outs = {}
        for form, fn in forms.items():
            legs[f"torch_{form}_fwd"] = lambda fn=fn: fn(Q, c)
            outs[form] = fn(Qg, cg)
            legs[f"torch_{form}_bwd"] = lambda form=form: torch.autograd.grad(outs[form], (Qg, cg), dy, retain_graph=True)
        for fn in legs.values():  # untimed round: allocations, kernel selection
            fn()
        torch.cuda.synchronize()
        Q64, c64, dy64 = Q.double(), c.double(), dy.double()
        parity = {"y": relerr(y, torch.einsum("bkn,bk->bn", Q64, c64)), "dQ": relerr(dQ, torch.einsum("bk,bn->bkn", c64, dy64)),
                  "dc": relerr(dc, torch.einsum("bkn,bn->bk", Q64, dy64))}
        del Q64
        times = {leg: [] for leg in legs}
        for _ in range(args.reps):
            for leg, fn in legs.items():
                times[leg].append(timed_ms(fn, args.inner))
        ms = {leg: statistics.median(v) for leg, v in times.items()}
        bytes_fwd = (p * k * n + p * n) * es
        bytes_bwd = (2 * p * k * n + p * n) * es
        line = {
            "shape": name, "n": n, "k": k, "p": p, "dtype": str(dt).replace("torch.", ""), "reps": args.reps, "inner": args.inner,
            "ms": {leg: round(v, 4) for leg, v in ms.items()},
            "ms_min_max": {leg: [round(min(v), 4), round(max(v), 4)] for leg, v in times.items()},
            "native_fwd_GBps": round(bytes_fwd / ms["native_fwd"] / 1e6, 1),
            "native_bwd_GBps": round(bytes_bwd / ms["native_bwd"] / 1e6, 1),
            "fwd_speedup_over_weighted": round(ms["torch_weighted_fwd"] / ms["native_fwd"], 2),
            "fwd_speedup_over_einsum": round(ms["torch_einsum_fwd"] / ms["native_fwd"], 2),
            "bwd_speedup_over_weighted": round(ms["torch_weighted_bwd"] / ms["native_bwd"], 2),
            "bwd_speedup_over_einsum": round(ms["torch_einsum_bwd"] / ms["native_bwd"], 2),
            "native_against_fp64_einsum_relerr": parity,
        }
        if args.krylov_gbps > 0:
            line["krylov_vector_hbm_GBps"] = args.krylov_gbps
            line["native_fwd_over_krylov_vector_hbm"] = round(line["native_fwd_GBps"] / args.krylov_gbps, 2)
            line["native_bwd_over_krylov_vector_hbm"] = round(line["native_bwd_GBps"] / args.krylov_gbps, 2)
        print(json.dumps(line), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
