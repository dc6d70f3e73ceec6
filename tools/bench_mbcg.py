"""One value-and-gradient of the GP log-density by modified batched CG (gp_util.logpdf_mbcg) against the SLQ + PCG path
(gp_util.logpdf_krylov_p: krylov_logdet_slq with lanczos.integrand_spd beside a separate pcg solve), at BASELINE config 2: all
45 730 rows of the UCI protein inputs (tests/golden/uci_protein_X.npz), d = 9, ARD Matern-3/2, fp32, 8 probes, k = 30 matvecs, without
a preconditioner and with a pivoted-Cholesky one of rank --rank.

Both paths get the same operator, targets, mean and the same prebuilt preconditioner; they are timed in alternation in one process
(A B A B ...), each value-and-gradient bracketed by hipEvents on the current stream; medians of --reps.  Peak device memory of each
path: torch's allocator peak over one value-and-gradient, started from an empty scratch cache.

  python tools/bench_mbcg.py [--reps R] [--rank RANK] [--k K] [--probes P] [--rows N]

One JSON line per preconditioner setting on stdout."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from matfree_extensions import _lib, cg, hutchinson, low_rank  # noqa: E402
from matfree_extensions.operators import RbfGramOp  # noqa: E402
from matfree_extensions.util import gp_util  # noqa: E402


def timed_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def peak_mib(fn, dev):
    torch.cuda.synchronize()
    _lib._ws_cache.clear()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rank", type=int, default=50)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--probes", type=int, default=8)
    ap.add_argument("--rows", type=int, default=0, help="use only the first N rows (0: all)")
    args = ap.parse_args()
    dev, dt = torch.device("cuda:0"), torch.float32
    X = np.load(os.path.join(ROOT, "tests", "golden", "uci_protein_X.npz"))["X"]
    if args.rows:
        X = X[: args.rows]
    n, d = X.shape
    rng = np.random.default_rng(0)
    y = np.sin(X @ (rng.standard_normal(d) / 3.0)) + 0.1 * rng.standard_normal(n)
    X, y = torch.tensor(X, dtype=dt, device=dev), torch.tensor(y, dtype=dt, device=dev)
    raw = [torch.zeros(d, dtype=dt, device=dev, requires_grad=True)] + [torch.zeros((), dtype=dt, device=dev, requires_grad=True) for _ in range(2)]
    const = torch.zeros((), dtype=dt, device=dev, requires_grad=True)
    op = RbfGramOp(X, noise_minval=1e-4, kernel="matern32")
    leaves = [*raw, const]

    for rank in (0, args.rank):
        cov = op.bind(*raw)
        P = None
        if rank:
            pre, _ = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=rank))(low_rank.without_noise(cov), n)
            P = pre.bind((1e-4 + torch.nn.functional.softplus(raw[2])).detach())
        mbcg = gp_util.logpdf_mbcg(cg.mbcg_fixed_step(args.k), num_probes=args.probes)
        sample = hutchinson.sampler_rademacher(y, num=args.probes)
        slq = gp_util.krylov_logdet_slq(args.k, sample=sample, num_batches=1)
        if rank:
            krylov = gp_util.logpdf_krylov_p(cg.pcg_fixed_step(args.k), slq)
        else:
            krylov = gp_util.logpdf_krylov(cg.cg_fixed_step(args.k), slq)

        def run(logpdf, key):
            kw = {"P": P} if (rank or logpdf is mbcg) else {}
            value, _ = logpdf(y, key, mean=const.expand(n), cov_matvec=op.bind(*raw), **kw)
            torch.autograd.grad(value, leaves)
            return value

        values = {"mbcg": float(run(mbcg, 1)), "slq_pcg": float(run(krylov, 1))}  # warm-up: workspaces, hipGraph capture
        run(mbcg, 1), run(krylov, 1)
        torch.cuda.synchronize()
        times = {"mbcg": [], "slq_pcg": []}
        for rep in range(args.reps):
            times["mbcg"].append(timed_ms(lambda: run(mbcg, 2 + rep)))
            times["slq_pcg"].append(timed_ms(lambda: run(krylov, 2 + rep)))
        peaks = {"mbcg": peak_mib(lambda: run(mbcg, 1), dev), "slq_pcg": peak_mib(lambda: run(krylov, 1), dev)}
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({"config": "C2 UCI protein", "n": n, "d": d, "kernel": "matern32 ARD", "dtype": "fp32", "k": args.k,
                          "probes": args.probes, "precond_rank": rank, "reps": args.reps,
                          "mbcg_value_and_grad_ms": round(med["mbcg"], 2), "slq_pcg_value_and_grad_ms": round(med["slq_pcg"], 2),
                          "mbcg_ms_all": [round(t, 2) for t in times["mbcg"]], "slq_pcg_ms_all": [round(t, 2) for t in times["slq_pcg"]],
                          "speedup": round(med["slq_pcg"] / med["mbcg"], 2), "mbcg_peak_MiB": round(peaks["mbcg"], 1),
                          "slq_pcg_peak_MiB": round(peaks["slq_pcg"], 1), "logpdf_per_n": {k: v / n for k, v in values.items()},
                          "device": torch.cuda.get_device_name(0)}), flush=True)
    assert math.isfinite(sum(values.values()))


if __name__ == "__main__":
    main()
