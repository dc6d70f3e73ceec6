"""Headline benchmark: SLQ log-det value-and-gradient for a matrix-free RBF GP kernel (BASELINE config 4).

    python bench.py --gpus N --steps K --warmup W [--scaling strong|weak] [--row-group R] [--dump-outputs DIR] [--full]

N > 1 either under a launcher (python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...:
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* come from the environment) or stand-alone: `python bench.py --gpus N` then starts
the N ranks itself as child processes, BEFORE anything in the parent touches a GPU.

One "step" = one SLQ log-determinant value AND gradient w.r.t. (raw_lengthscale, raw_outputscale, raw_noise):
40 fully re-orthogonalised Lanczos steps (forward), the k x k eigen-quadrature, the Arnoldi adjoint scan (40 more Gram
matvecs) and the deferred parameter-gradient sweep, then the fused all-reduce of [sum q, sum q^2, sum dq/dtheta].
Operator: X ~ N(0,1) of shape (131072, 8), lengthscale 2, outputscale 1, noise 0.1, fp32.

  --scaling strong (default): BASELINE config 4 as written -- 64 probes in TOTAL on N GPUs.  The rows of the kernel matrix and
      of every Krylov vector are sharded over the N ranks (all 64 probes on every rank): per Krylov step one all-gather of the
      iterate and two or three small all-reduces of Gram-Schmidt coefficients.  --row-group R < N makes R-rank row groups
      and shards the probes over the N / R groups.
  --scaling weak: 64 probes PER GPU, probes sharded, operator replicated, one all-reduce per step.

A plain run sets up, warms up, times the K steps and prints ONE JSON line on rank 0 (DESIGN.md section 4 explains the fields).
--full adds what takes runs of its own: the timed steps repeated under libmfx's kernel timers (roofline, per-kernel breakdown),
the other two arithmetic modes, the gather legs of a row group (N > 1) and the CPU baseline (N = 1).
--dump-outputs DIR writes what the last timed step returned (estimate, spread over probes, the three gradients) as DIR/<name>.npy;
the inputs depend on the arguments only, so two builds can be compared output for output.
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "experiments-lanczos-adjoints_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32-input MFMA = fp32 vector peak
MFMA_F16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: BF16/FP16 MFMA ~2.5 PF dense
MODES = ("f16x3", "f16x3-matvec", "fp32")
DEFAULT_MODE = "f16x3"


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="strong: --probes in total over all GPUs, rows sharded (BASELINE config 4); weak: --probes per GPU, probes sharded")
    ap.add_argument("--probes", type=int, default=64, help="probes in total (strong) or per GPU (weak)")
    ap.add_argument("--probes-per-gpu", type=int, default=None, help="alias of --scaling weak --probes P")
    ap.add_argument("--row-group", type=int, default=0, help="strong scaling: ranks per row group (0 = all ranks: pure row sharding)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-modes", action="store_true", help="--full: skip the timings of the other two arithmetic modes")
    ap.add_argument("--cpu-sample-n", type=int, default=0, help="0 = 8192 (smaller on a host where that would exceed ~30 s per run)")
    ap.add_argument("--kernel", default="rbf", choices=["rbf", "matern32", "matern12"],
                    help="kernel family (BASELINE config 4 is the RBF kernel; the reference's UCI runs use matern32)")
    ap.add_argument("--precision", default=DEFAULT_MODE, choices=list(MODES),
                    help="arithmetic of the fp32 Gram kernels (DESIGN.md section 3.2): f16x3 = matvec and gradient GEMM emulated on the "
                         "f16 matrix pipe (3 products, fp32 accumulate); f16x3-matvec = exact fp32 gradient GEMM; fp32 = exact fp32 MFMA")
    ap.add_argument("--stub", default="", help="(tests) run the launcher / collection logic on this backend without any GPU work")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend of the N > 1 run (nccl = RCCL; gloo only to rehearse "
                                                      "the multi-rank path on a box with fewer GPUs than ranks)")
    ap.add_argument("--gather", default="", choices=["", "grouped", "packed"],
                    help="native RCCL row group: how the iterate is all-gathered per Krylov step (include/mfx.h MFX_GATHER_*; default packed)")
    ap.add_argument("--share-gpus", action="store_true", help="(rehearsal) ranks beyond the visible GPUs share them (needs --backend gloo)")
    ap.add_argument("--full", action="store_true", help="also the kernel-timer repeat (roofline, breakdown), the other arithmetic modes, "
                                                        "the gather legs (N > 1) and the CPU baseline (N = 1)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the last timed step returned as DIR/<name>.npy")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.probes_per_gpu is not None:
        args.scaling, args.probes = "weak", args.probes_per_gpu
    return args


def inv_softplus(x):
    import numpy as np

    return float(np.log(np.expm1(x)))


def dump_outputs(folder, out):
    """--dump-outputs: the (mean, std, grads) a step returns, as computed (fp64 estimate and spread, fp32 gradients)."""
    import numpy as np

    mean, std, grads = out
    arrays = {"logdet_mean": mean, "probe_std": std}
    arrays.update(zip(("grad_raw_lengthscale", "grad_raw_outputscale", "grad_raw_noise"), grads))
    os.makedirs(folder, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(folder, name + ".npy"), t.detach().cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` without a launcher starts its own ranks (the parent never touches a GPU)
# ------------------------------------------------------------------------------------------------------------------------
def launch_children(args, argv):
    """Start the ranks, watch ALL of them: the first rank that dies takes the others with it (a rank that fails at start-up --
    --gpus beyond the device count, an RCCL init error -- must not leave its peers waiting in the rendezvous until the
    time-out).  Rendezvous through a file store owned by the parent: no port to lose between choosing it and binding it."""
    import tempfile

    store = tempfile.NamedTemporaryFile(prefix="mfx_bench_store_", delete=False)
    store.close()
    os.unlink(store.name)  # torch's FileStore creates it
    procs = []
    for rank in range(args.gpus):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(args.gpus), MFX_BENCH_INIT=f"file://{store.name}",
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        # rank 0 inherits stdout (its JSON line is the result); the others keep stderr only
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env,
                                      stdout=None if rank == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        live = list(procs)
        while live:
            time.sleep(0.2)
            for pr in list(live):
                code = pr.poll()
                if code is None:
                    continue
                live.remove(pr)
                if code != 0 and rc == 0:
                    rc = code
                    for other in live:  # exact PIDs of our own children
                        other.terminate()
            if rc != 0 and live:
                deadline = time.time() + 10
                for other in live:
                    try:
                        other.wait(timeout=max(0.1, deadline - time.time()))
                    except subprocess.TimeoutExpired:
                        other.kill()
                live = []
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
        try:
            os.unlink(store.name)
        except OSError:
            pass
    return rc


# ------------------------------------------------------------------------------------------------------------------------
# CPU baseline
# ------------------------------------------------------------------------------------------------------------------------
def cpu_baseline(args):
    """The oracle (NumPy port of the reference algorithm, kind "port") on a bounded sample of the same workload: identical
    d, k and hyper-parameters, ONE probe, n reduced to 8192 (6 % of N; ~4 s per run on the 16 host cores of the 1-GPU box).
    Protocol: one warm-up, then the MEDIAN of 5 timed runs at the sample size.  The full-size figure is the
    n^2 extrapolation of the sample (the Gram work dominates at N); the exponent fitted from two measured sizes (the 2048-point
    calibration run and the sample) and the figure it would give are in `scaling_fit`."""
    import math

    import numpy as np
    from threadpoolctl import threadpool_limits

    from oracle import slq_oracle as orc

    raw = tuple(np.float32(v) for v in (inv_softplus(2.0), inv_softplus(1.0), inv_softplus(0.1)))
    threads = min(16, len(os.sched_getaffinity(0)))  # the 1-GPU box's CPU share is 16 cores

    def once(ns):
        rng = np.random.default_rng(4)
        X = rng.standard_normal((ns, args.d)).astype(np.float32)
        probes = orc.rademacher(5, 1, ns, dtype=np.float32)
        t0 = time.perf_counter()
        orc.hutchinson_value_and_grad(orc.RbfGramOp(X, cache_limit=0), args.k, probes, raw)
        return time.perf_counter() - t0

    with threadpool_limits(limits=threads):
        n_cal = 2048
        once(n_cal)
        t_cal = sorted(once(n_cal) for _ in range(3))[1]
        ns = args.cpu_sample_n if args.cpu_sample_n > 0 else 8192
        if args.cpu_sample_n <= 0 and t_cal * (ns / n_cal) ** 2 > 30.0:  # a slow host: keep the whole leg near a minute
            ns = int(n_cal * (30.0 / t_cal) ** 0.5) // 512 * 512
        once(ns)  # warm-up
        times = sorted(once(ns) for _ in range(5))
    med = times[2]
    measured = 1.0 / med
    expo = math.log(med / t_cal) / math.log(ns / n_cal) if ns > n_cal else 2.0
    # value: the plain n^2 extrapolation (the Gram work dominates at N = 131072; the exponent fitted from two small sizes comes out
    # near 2.1-2.2 because non-quadratic costs still show at n = 2048 -- that figure is the secondary field)
    return {
        "value": measured * (ns / args.n) ** 2,
        "unit": "probes/s",
        "cores": threads,
        "kind": "port",
        "measured_at_sample": {"n": ns, "probes_per_s": measured, "seconds_median_of_5": med, "seconds_all": times},
        "scaling_fit": {"n_small": n_cal, "seconds_small_median_of_3": t_cal, "n_sample": ns, "seconds_sample": med, "exponent": expo,
                        "value_with_fitted_exponent": measured * (ns / args.n) ** expo},
        "sample": f"NumPy oracle (matrix-free kernel, re-evaluated per matvec), 1 probe, k={args.k}, d={args.d}, n={ns} (of {args.n}): "
                  f"1 warm-up + median of 5 runs = {med:.2f} s = {measured:.4f} probes/s at n={ns}; value = that x (n_sample/n)^2 "
                  f"(exponent fitted from the runs at n={n_cal} ({t_cal:.2f} s) and n={ns}: {expo:.2f}); BLAS threads={threads}",
    }


# ------------------------------------------------------------------------------------------------------------------------
# one rank
# ------------------------------------------------------------------------------------------------------------------------
def run_stub(args, world, rank):
    """launcher / collection logic without a GPU (tests/test_bench_launcher.py): rendezvous, barrier, max over ranks, one line"""
    import torch
    import torch.distributed as dist

    if world > 1:
        how = {}
        if os.environ.get("MFX_BENCH_INIT"):
            how = dict(init_method=os.environ["MFX_BENCH_INIT"], rank=rank, world_size=world)
        dist.init_process_group(args.stub, **how)
        dist.barrier()
    t = torch.tensor([0.001 * (rank + 1)], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.barrier()
    if rank == 0:
        p_total = args.probes if args.scaling == "strong" else args.probes * world
        print(json.dumps({"metric": "stub", "value": p_total / t.item(), "n_gpus": world, "scaling": args.scaling,
                          "config": {"probes_total": p_total, "world_size_seen_by_rank0": dist.get_world_size() if world > 1 else 1}}))
    if world > 1:
        dist.destroy_process_group()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch_children(args, argv))
    world = int(env_world or "1")
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a number for another world size")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.stub:
        return run_stub(args, world, rank)

    import numpy as np  # noqa: F401
    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (there is no CPU product path)")
    if args.share_gpus:
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")
    if world > 1:
        import datetime

        limit = datetime.timedelta(seconds=180)  # a rank that dies must not leave the others waiting in a collective for long
        how = {}
        if os.environ.get("MFX_BENCH_INIT"):  # started by launch_children: the parent's file store (a launcher sets MASTER_*)
            how = dict(init_method=os.environ["MFX_BENCH_INIT"], rank=rank, world_size=world)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=limit, **how)  # nccl == RCCL on ROCm; one rank per GPU
        else:
            dist.init_process_group(args.backend, timeout=limit, **how)

    if args.gather:
        os.environ["MFX_GATHER"] = args.gather
    from matfree_extensions import _lib, hutchinson, lanczos
    from matfree_extensions.distributed import Layout, reduce_estimate, shard_probes
    from matfree_extensions.operators import RowShardedOp
    from matfree_extensions.util import gp_util

    n, d, k = args.n, args.d, args.k
    strong = args.scaling == "strong"
    p_total = args.probes if strong else args.probes * world
    row_group = (args.row_group or world) if strong else 1
    layout = Layout(n, row_group if world > 1 else 1)
    first, count = shard_probes(p_total, layout.probe_index, layout.probe_groups)
    gen = torch.Generator().manual_seed(4)
    X = torch.randn((n, d), generator=gen, dtype=torch.float32).to(dev)
    params = [torch.tensor(v, dtype=torch.float32, device=dev, requires_grad=True)
              for v in (inv_softplus(2.0), inv_softplus(1.0), inv_softplus(0.1))]
    sampler = hutchinson.sampler_rademacher(X[:, 0], num=count)

    def make_step(precision, comm=layout.comm):
        op = gp_util.gram_operator(X, precision=precision, kernel=args.kernel)
        matvec = RowShardedOp(op, comm) if comm is not None else op
        integrand = lanczos.integrand_spd(torch.log, k, matvec)

        def step(seed):
            probes = sampler((seed, first))  # this probe group's slice of ONE global +-1 probe matrix
            if comm is not None:
                probes = comm.rows(probes)
            values = integrand(probes, *params)
            grads = torch.autograd.grad(values.sum(), params)
            return reduce_estimate(values.detach(), grads, p_total, replicas=layout.replicas)

        return step

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(step, steps, warmup):
        out = None
        for w in range(warmup):
            out = step(100 + w)
        fence()
        t0 = time.perf_counter()
        for s in range(steps):
            out = step(s)
        fence()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.item(), out

    # The timed region runs WITHOUT libmfx's per-launch hipEvent timers (they also switch the hipGraph replay off and cost 2.5 % at
    # the per-rank size of the 8-way shard, profiles/r03b_*): `ms_per_step` / `value` are timer-free for every N.  With --full the
    # same steps (same seeds) are then repeated with the timers on: the roofline figures and `breakdown_ms_per_step` come from that
    # pass, and its wall time is reported next to the headline.
    step = make_step(args.precision)
    for w in range(args.warmup):
        step(100 + w)
    fence()
    elapsed, out = timed(step, args.steps, 0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)
    rccl_view = None
    if world > 1 and layout.native:
        try:
            rccl_view = layout.comm.rccl_count()  # (ranks, rank) from ncclCommCount / ncclCommUserRank: RCCL's own view of the row group
        except Exception as exc:  # noqa: BLE001
            rccl_view = (f"unavailable ({exc})", None)
    if args.full:
        _lib.timing_reset()
        _lib.timing_enable(True)
        elapsed_timers, _ = timed(step, args.steps, 0)
        _lib.timing_enable(False)
        apply_ms, apply_cnt = _lib.timing_read(0)
        grad_ms, grad_cnt = _lib.timing_read(1)
        vec_ms, vec_cnt = _lib.timing_read(2)
        comm_ms, comm_cnt = _lib.timing_read(3)
        _lib.timing_reset()

    # --full: every gather leg of the row group in the SAME process group, so that one `bench.py --gpus N --full` line carries all of
    # them: the native communicator's packed and grouped all-gather (include/mfx.h MFX_GATHER_*) and the torch.distributed callbacks
    # (what MFX_NATIVE_COMM=0 selects).  Per leg: 1 warm-up + 2 timed steps without kernel timers, then one step with them for the
    # all-gather's own time.  The headline above is the leg named in `config.parallelism`.
    gather_legs = None
    if args.full and world > 1 and layout.comm is not None:
        from matfree_extensions.distributed import RowComm

        def leg(comm_obj):
            st = make_step(args.precision, comm_obj)
            t, _ = timed(st, 2, 1)
            _lib.timing_reset()
            _lib.timing_enable(True)
            timed(st, 1, 0)
            _lib.timing_enable(False)
            g_ms, _ = _lib.timing_read(3)
            _lib.timing_reset()
            return {"ms_per_step": 1e3 * t / 2, "allgather_incl_pack_unpack": g_ms}

        # (a leg that fails the same way on every rank -- a Python-level error -- is recorded and skipped: the headline above is already
        #  measured and must survive it; a failure inside a collective cannot be survived by anything)
        def try_leg(name, comm_obj):
            try:
                gather_legs[name] = leg(comm_obj)
            except Exception as exc:  # noqa: BLE001
                gather_legs[name] = {"error": f"{type(exc).__name__}: {exc}"}

        gather_legs = {}
        if layout.native:
            headline = layout.comm.gather
            for mode_name in ("packed", "grouped"):
                layout.comm.set_gather(mode_name)
                try_leg("native_" + mode_name, layout.comm)
            layout.comm.set_gather(headline)
        try_leg("torch_distributed_callbacks", RowComm(n, layout.comm.group))

    modes = {args.precision: 1e3 * elapsed / args.steps}
    if args.full and not args.no_modes:
        for mode in MODES:
            if mode != args.precision:
                t, _ = timed(make_step(mode), 2, 1)
                modes[mode] = 1e3 * t / 2

    if rank == 0:
        ms_per_step = 1e3 * elapsed / args.steps
        value = p_total * args.steps / elapsed
        rows_local = layout.comm.nrows if layout.comm is not None else n
        split = args.precision.startswith("f16x3")
        mean, std, grads = out
        if layout.native:
            collectives = (f"libmfx -> RCCL (native, {layout.comm.gather} gather); ranks in the communicator libmfx itself holds "
                           f"(ncclCommCount) = {rccl_view[0]}")
        else:
            collectives = "host callbacks" if layout.comm is not None else "none"
        line = {
            "metric": "slq_logdet_value_and_grad_throughput",
            "value": value,
            "unit": "probes/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32" if not split else "f32 (Gram contraction emulated with 3 f16 MFMA products, fp32 accumulate; accuracy vs "
                                             "fp64 at this size on 32 probe sets, profiles/r05b_accuracy_16_seeds/: value <= 5.6e-6 and d/d raw_noise <= 1.3e-5 on "
                                             "all 32; the other two gradient components <= 1e-4 on 25 of 32 sets, <= 1.5e-4 on 29, worst 3.96e-4 -- the 1e-4 gate "
                                             "is NOT met on every probe set; the estimator's own sampling error is 1.55e-3)",
            "data": "synthetic",
            "config": {
                "workload": f"matrix-free RBF GP kernel N={n} d={d}, SLQ log-det value+grad, {k} Lanczos steps (full reortho) x "
                            f"{p_total} probes, fp32 (BASELINE config 4)",
                "N": n, "d": d, "krylov_depth": k, "probes_total": p_total, "probes_on_this_rank": count,
                "rows_on_this_rank": rows_local,
                "parallelism": f"{layout.describe()}; world size seen by rank 0 (torch.distributed) = {dist.get_world_size() if world > 1 else 1}; "
                               f"row-group collectives: {collectives}",
                "rccl_comm_ranks": rccl_view[0] if rccl_view else None,
                "gram_precision": args.precision, "kernel": args.kernel,
            },
            "result": {"logdet_mean": float(mean), "probe_std": float(std), "grad": [float(g) for g in grads]},
        }
    if rank == 0 and args.full:
        # dominant kernel: the Gram matvec.  Algorithmic flops per launch: the contraction 2 rows n p on this rank (what the matrix
        # cores must deliver); distance + exp are extra work priced in DESIGN.md.
        flops_launch = 2.0 * rows_local * n * count
        avg_ms = apply_ms / max(apply_cnt, 1)
        achieved = flops_launch / (avg_ms * 1e-3) / 1e12 if apply_cnt else 0.0
        peak = MFMA_F16_PEAK_TFLOPS if split else MFMA_F32_PEAK_TFLOPS
        kernel = ("k_rbf_fat_apply (Gram matvec, one wave per SIMD; fp32 emulated by 3 f16 MFMA products, distances included; "
                  "pre-pass and split reduction inside the timed span)" if split else "k_rbf_mfma_apply (Gram matvec, exact fp32 MFMA)")
        # HBM-side bytes per launch: NOT measured in this run (PMC counters need rocprofv3 around the process) -- read from the file
        # tools/prof_traffic.sh wrote, which names the commit and the command it was collected on (`traffic_source`)
        traffic, traffic_source = None, None
        tfile = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tfile) and world == 1:
            tj = json.load(open(tfile))
            traffic = tj.get("k_rbf_fat_apply_hbm_bytes_per_launch" if split else "k_rbf_mfma_apply_hbm_bytes_per_launch")
            traffic_source = f"profiles/traffic.json @ {tj.get('commit', 'unknown commit')} ({tj.get('command', 'command not recorded')}); read from the file, not measured in this run"
        batch = count * k
        line.update({
            "ms_per_step_with_kernel_timers": 1e3 * elapsed_timers / args.steps,
            "modes": {"ms_per_step": modes,
                      "note": "same process, same inputs; the timed mode has --steps steps, the others 2 steps after 1 warm-up"},
            "roofline": {
                "kernel": kernel + f", {apply_cnt // max(args.steps, 1)} launches per step",
                "bound": "mfma",
                "achieved": achieved,
                "peak": peak,
                "unit": "TFLOP/s",
                "frac": achieved / peak,
                "traffic": traffic,
                "traffic_source": traffic_source,
                "avg_launch_ms": avg_ms,
                "launches": apply_cnt,
                "measured_in": "the instrumented repeat of the timed steps (same seeds, hipEvents around every launch of the class on the "
                               "stream it is launched on); the timed region itself runs without timers",
                "algorithmic_flops_per_launch": flops_launch,
                # the 3-product emulation executes 3x the algorithmic MFMA flops: its ceiling is peak / 3
                "executed_mfma_flops_factor": 3.0 if split else 1.0,
                "frac_of_fp32_mfma_peak": achieved / MFMA_F32_PEAK_TFLOPS,
            },
            "gather_legs_ms_per_step": gather_legs,
            "breakdown_ms_per_step": {
                "gram_matvec": apply_ms / args.steps,
                "param_grad_sweep": grad_ms / args.steps,
                "krylov_vector_kernels": vec_ms / args.steps,
                "allgather_incl_pack_unpack": comm_ms / args.steps,  # (the small all-reduces sit inside krylov_vector_kernels)
            },
            "param_grad_gemm": {
                # S = L^T R over all (probe, step) pairs of this rank: algorithmic flops 2 rows n batch, once per step
                "algorithmic_flops": 2.0 * rows_local * n * batch,
                "achieved_TFLOPs": 2.0 * rows_local * n * batch / max(grad_ms / max(grad_cnt, 1) * 1e-3, 1e-12) / 1e12,
                "peak_TFLOPs": MFMA_F16_PEAK_TFLOPS if args.precision == "f16x3" else MFMA_F32_PEAK_TFLOPS,
                "executed_mfma_flops_factor": 3.0 if args.precision == "f16x3" else 1.0,
                "note": "f16x3: the batch rows are packed by decreasing size and the tail that holds <= 2^-10 of the summed row bounds "
                        "|L_b|max |R_b|max is multiplied hi*hi only (what that drops is bounded by 2^-20 of the summed bounds, the size of what "
                        "the three-product sum drops anyway; decided on the device per launch, DESIGN.md section 3.3) -- the executed factor is 3 "
                        "for the other rows" if args.precision == "f16x3" else "",
            },
            "krylov_vector_hbm": {
                # B_fwd + B_bwd = p n s [2k(k+1)+3k] + p n s [3k^2+9k] algorithmic bytes (this rank's rows)
                "algorithmic_GB_per_step": count * rows_local * 4 * (2 * k * (k + 1) + 3 * k + 3 * k * k + 9 * k) / 1e9,
                "achieved_GBps": (count * rows_local * 4 * (2 * k * (k + 1) + 3 * k + 3 * k * k + 9 * k) / 1e9)
                                 / max(vec_ms / args.steps * 1e-3, 1e-12),
                "peak_GBps": HBM_PEAK_GBS,
            },
        })
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(args)
    if rank == 0:
        print(json.dumps(line))
    if world > 1:
        # the native communicator goes before the process group does (ncclCommDestroy from __del__ at interpreter shutdown would run
        # in a different order on every rank)
        dist.barrier()
        if layout.comm is not None and getattr(layout, "native", False):
            layout.comm.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
