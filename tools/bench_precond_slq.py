"""Preconditioned SLQ at the shapes of BASELINE config 4 (X ~ N(0, 1), n = 131 072, d = 8, lengthscale 2,
noise 0.1, 64 probes) and config 2 (n = 45 730, d = 9, 8 probes; synthetic z-scored inputs stand in for the protein file, which the
timing does not depend on), fp32.

  apply   mfx_lowrank_apply against mfx_precond_apply (whose kernels this change leaves alone) on the same factor and vectors, for
          p in {8, 64} and rank in {32, 64, 128}: both in one process, timed in alternation (A B A B ...), one window = --inner
          back-to-back calls between two hipEvents, median [min, max] over --reps windows after one untimed round.
  step    one SLQ value-and-gradient step: plain at depth 40 against preconditioned (rank --rank partial Cholesky of the noise-free
          kernel) at depths 10, 20 and 40, with the mean and the per-probe standard deviation of both estimates beside the times
          (median of --reps steps; host wall time, each step ended by a synchronise).

One JSON line per measurement on stdout.

  python tools/bench_precond_slq.py [--config 4] [--reps 5] [--inner 10] [--rank 64] [--n N] [--skip-step]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
import torch  # noqa: E402
from matfree_extensions import _lib, lanczos, low_rank  # noqa: E402
from matfree_extensions.operators import PreconditionedOp, RbfGramOp  # noqa: E402

CONFIGS = {4: dict(n=131072, d=8, p=64, lengthscale=2.0, noise=0.1), 2: dict(n=45730, d=9, p=8, lengthscale=1.0, noise=0.1)}


def timed_ms(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def alternate(fns, reps, inner):
    for fn in fns.values():
        timed_ms(fn, 1)
    samples = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            samples[name].append(timed_ms(fn, inner))
    return {name: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for name, v in samples.items()}


def bench_apply(n, p, rank, reps, inner, dev):
    lib, dt, code = _lib.get(), torch.float32, _lib.MFX_F32
    gen = torch.Generator(device="cpu").manual_seed(rank)
    pre = low_rank.Preconditioner((torch.randn((n, rank), generator=gen) / math.sqrt(n)).to(dev))
    V = torch.randn((p, n), generator=gen).to(dev)
    minv, s = pre.minv(0.1)
    scale = (1.0 / s).contiguous()
    z0, z1 = torch.empty_like(V), torch.empty_like(V)
    desc = _lib.Operator()
    desc.kind, desc.dtype, desc.n = _lib.OP_DENSE, code, n
    ws0 = torch.empty(int(lib.mfx_pcg_workspace_bytes(C.byref(desc), n, p, rank)), dtype=torch.uint8, device=dev)
    ws1 = torch.empty(int(lib.mfx_lowrank_workspace_bytes(code, n, rank, p)), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    fns = {
        "mfx_precond_apply": lambda: _lib.check(lib.mfx_precond_apply(code, n, rank, _lib.ptr(pre.lt), _lib.ptr(minv), _lib.ptr(s),
                                                                      _lib.ptr(V), n, _lib.ptr(z0), n, p, _lib.ptr(ws0), ws0.numel(), st)),
        "mfx_lowrank_apply": lambda: _lib.check(lib.mfx_lowrank_apply(code, n, rank, _lib.ptr(pre.lt), _lib.ptr(minv), _lib.ptr(scale),
                                                                      _lib.ptr(V), n, _lib.ptr(z1), n, p, _lib.ptr(ws1), ws1.numel(), st)),
    }
    ms = alternate(fns, reps, inner)
    agree = float((z0.double() - z1.double()).abs().max() / z0.double().abs().max())
    es = 4
    return {"what": "apply", "n": n, "p": p, "rank": rank, "ms": ms, "rel_diff": agree,
            "lt_bytes": {"mfx_precond_apply": 2 * p * rank * n * es, "mfx_lowrank_apply": 2 * ((p + 15) // 16) * rank * n * es}}


def slq_step(bound, V, k):
    """-> (host wall-clock ms between two synchronises, per-probe values) of one value-and-gradient step"""
    leaves = [q.detach().clone().requires_grad_(True) for q in bound.params]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    values = lanczos.integrand_spd(torch.log, k, bound.op.bind(*leaves))(V)
    values.mean().backward()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, values.detach().double()


def bench_step(cfg, rank, reps, dev):
    n, d, p = cfg["n"], cfg["d"], cfg["p"]
    gen = torch.Generator(device="cpu").manual_seed(4)
    X = torch.randn((n, d), generator=gen).to(dev)
    inv_sp = lambda v: math.log(math.expm1(v))  # noqa: E731
    raw = [torch.tensor(inv_sp(v), device=dev) for v in (cfg["lengthscale"], 1.0, cfg["noise"])]
    op = RbfGramOp(X)
    A = op.bind(*raw)
    V = torch.sign(torch.randn((p, n), generator=gen)).to(dev)
    pre, info = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=rank))(low_rank.without_noise(A), n)
    B = PreconditionedOp(op, pre, torch.tensor(cfg["noise"], device=dev))
    logdet_p = float(B.logdet())
    out = []
    for name, bound, k, shift in [("plain", A, 40, 0.0)] + [("preconditioned", B.bind(*raw), k, logdet_p) for k in (10, 20, 40)]:
        slq_step(bound, V, k)  # untimed
        runs = [slq_step(bound, V, k) for _ in range(reps)]
        vals = runs[-1][1] + shift
        out.append({"what": "step", "estimator": name, "n": n, "p": p, "k": k, "rank": rank if name != "plain" else 0,
                    "ms": round(statistics.median(r[0] for r in runs), 3), "mean": float(vals.mean()),
                    "std_per_probe": float(vals.std(unbiased=False)), "finite": bool(torch.isfinite(vals).all())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4, choices=sorted(CONFIGS))
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    cfg = dict(CONFIGS[args.config])
    if args.n:
        cfg["n"] = args.n
    dev = torch.device("cuda:0")
    for p in (8, 64):
        for rank in (32, 64, 128):
            print(json.dumps(bench_apply(cfg["n"], p, rank, args.reps, args.inner, dev)), flush=True)
    if not args.skip_step:
        for row in bench_step(cfg, args.rank, args.reps, dev):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
