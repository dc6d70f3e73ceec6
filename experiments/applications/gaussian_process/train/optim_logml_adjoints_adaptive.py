"""GP hyper-parameter training (UCI-style regression) on the Krylov log-marginal likelihood, adaptive PCG.

Same structure, flags and outputs as the reference's `optim_logml_adjoints_adaptive.py` (Matern-3/2 ARD kernel, constant
mean, rank-`rank_precon` pivoted-Cholesky preconditioner, PCG stopped at `cg_tol`, SLQ log-determinant with
`num_matvecs` Lanczos steps x `num_samples` Rademacher probes, Adam 0.05; wall-clock per epoch in
`*_loss_timestamps.npy`).  Differences: the `num_samples` probes are ONE native batch (one Gram sweep serves them all)
instead of sequential single-probe batches; `--num_partitions` only rounds the data size like the reference does (no
Gram tile ever reaches HBM); without the dataset on disk (`./data/uci/<name>/data.csv.gz`) a synthetic set of the same
shape is generated (`protein`: 45 730 x 9).
"""

import argparse
import gzip
import os
import sys
import time

import numpy as np
import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "../../../.."))
sys.path.insert(0, os.path.join(_ROOT, "experiments-lanczos-adjoints_amd"))

from matfree_extensions import cg, hutchinson, low_rank  # noqa: E402
from matfree_extensions.util import exp_util, gp_util  # noqa: E402

_SHAPES = {"protein": (45730, 9), "kin40k": (40000, 8), "elevators": (16599, 18), "kegg_directed": (48827, 20),
           "kegg_undirected": (63608, 27), "concrete": (1030, 8), "power_plant": (9568, 4)}


def load_data(which, seed):
    path = f"./data/uci/{which}/data.csv.gz"
    if os.path.exists(path):
        with gzip.open(path, "rt") as f:
            arr = np.loadtxt(f, delimiter=",", skiprows=1)
        inputs, targets = arr[:, :-1], arr[:, -1]
    else:
        n, d = _SHAPES[which]
        if d > 16:
            raise SystemExit(f"{which}: d = {d} > 16 is outside the matrix-core Gram kernels of this build")
        rng = np.random.default_rng(seed)
        inputs = rng.standard_normal((n, d))
        w = rng.standard_normal(d) / np.sqrt(d)
        targets = np.sin(inputs @ w) + 0.5 * np.tanh(inputs[:, 0] * inputs[:, 1]) + 0.1 * rng.standard_normal(n)
        print(f"(synthetic stand-in for '{which}': {n} x {d})")
    inputs = (inputs - inputs.mean(0)) / (inputs.std(0) + 1e-6)
    targets = (targets - targets.mean()) / targets.std()
    return inputs, targets


parser = argparse.ArgumentParser()
parser.add_argument("--name", type=str, required=True)
parser.add_argument("--seed", type=int, required=True)
parser.add_argument("--dataset", type=str, required=True)
parser.add_argument("--rank_precon", type=int, required=True)
parser.add_argument("--num_partitions", type=int, required=True)
parser.add_argument("--num_matvecs", type=int, required=True)
parser.add_argument("--num_samples", type=int, required=True)
parser.add_argument("--num_epochs", type=int, required=True)
parser.add_argument("--cg_tol", type=float, required=True)
parser.add_argument("--precision", type=str, default="f16x3")
# SLQ on P^-1/2 A P^-1/2 plus log det P (gp_util.krylov_logdet_slq_p): the same log-determinant at a small --num_matvecs
parser.add_argument("--precond_slq", action="store_true")
args = parser.parse_args()
print(args)

dev, dt = torch.device("cuda:0"), torch.float32
noise_minval = 1e-4
train_test_split = 0.8
inputs, targets = load_data(args.dataset, args.seed)
coeff = len(inputs) // (5 * args.num_partitions)
num_data = int(coeff * 5 * args.num_partitions)
perm = np.random.default_rng(args.seed).permutation(num_data)
ntrain = int(train_test_split * num_data)
tr, te = perm[:ntrain], perm[ntrain:]
train_x, train_y = torch.as_tensor(inputs[tr], dtype=dt, device=dev), torch.as_tensor(targets[tr], dtype=dt, device=dev)
test_x, test_y = torch.as_tensor(inputs[te], dtype=dt, device=dev), torch.as_tensor(targets[te], dtype=dt, device=dev)
print("Train:", tuple(train_x.shape), "Test:", tuple(test_x.shape))

constrain = gp_util.constraint_greater_than(noise_minval)
gram_matvec = gp_util.gram_matvec_partitioned(args.num_partitions, checkpoint=True, precision=args.precision)
rank_precon = int(min(args.rank_precon, ntrain))
precondition = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=rank_precon))
ndim = train_x.shape[-1]
m, p_mean = gp_util.mean_constant(shape_out=())
k, p_kernel = gp_util.kernel_scaled_matern_32(shape_in=(ndim,), shape_out=())
prior = gp_util.model_gp(m, k)


def make_loss(n, cg_atol, maxiter):
    solve_p = cg.pcg_adaptive(rtol=0.0, atol=cg_atol, maxiter=maxiter, miniter=10)
    sample = hutchinson.sampler_rademacher(torch.ones(n, dtype=dt, device=dev), num=args.num_samples)
    if args.precond_slq:
        logdet_p = gp_util.krylov_logdet_slq_p(args.num_matvecs, sample=sample, num_batches=1)
        logpdf_p = gp_util.logpdf_krylov_pslq(solve_p=solve_p, logdet_p=logdet_p)
    else:
        logdet = gp_util.krylov_logdet_slq(args.num_matvecs, sample=sample, num_batches=1, checkpoint=True)
        logpdf_p = gp_util.logpdf_krylov_p(solve_p=solve_p, logdet=logdet)
    likelihood, p_likelihood = gp_util.likelihood_pdf_p(gram_matvec, logpdf_p, precondition, constrain=constrain)
    return gp_util.target_logml(prior, likelihood), p_likelihood


loss, p_likelihood = make_loss(ntrain, args.cg_tol, 1000)
ps = exp_util.tree_random_like(args.seed, (p_mean, p_kernel, p_likelihood))
ps = tuple({q: v.to(device=dev, dtype=dt).requires_grad_(True) for q, v in d.items()} for d in ps)
leaves = [v for d in ps for v in d.values()]


def mll_lanczos(loss_fun, key, Xs, ys):
    val, info = loss_fun(Xs, ys, key, params_mean=ps[0], params_kernel=ps[1], params_likelihood=ps[2])
    return -1.0 * val / len(Xs), info


def value_and_grad(key):
    for q in leaves:
        q.grad = None
    value, info = mll_lanczos(loss, key, train_x, train_y)
    value.backward()
    return value.detach(), info


def predict_mean(x):
    solve_ = cg.pcg_adaptive(atol=1e-2, rtol=0.0, maxiter=10_000, miniter=10)
    lik, _ = gp_util.likelihood_condition_p(gram_matvec, solve_, precondition=precondition, constrain=constrain)
    det = tuple({q: v.detach() for q, v in d.items()} for d in ps)
    postmean, _ = gp_util.target_posterior(prior, lik)(train_x, train_y, det[0], det[1], det[2])
    return postmean(x)


optimizer = torch.optim.Adam(leaves, lr=0.05)
value, aux = value_and_grad(args.seed)  # first call (workspace allocation; nothing to compile)
torch.cuda.synchronize()

loss_timestamps, loss_curve, cg_errors, cg_numsteps_all = [], [float(value)], [], []
start = time.perf_counter()
for epoch in range(args.num_epochs):
    value, aux = value_and_grad(args.seed + 1 + epoch)
    optimizer.step()
    residual = aux["logpdf"]["solve"]["residual_abs"]
    cg_error = float(torch.linalg.vector_norm(residual) / np.sqrt(residual.numel()))
    cg_numsteps = int(aux["logpdf"]["solve"]["num_steps"])
    loss_curve.append(float(value))
    loss_timestamps.append(time.perf_counter() - start)
    cg_errors.append(cg_error)
    cg_numsteps_all.append(cg_numsteps)
    print(f"epoch {epoch}: loss: {float(value):.3F}, cg_error: {cg_error:.1e}, cg_numsteps: {cg_numsteps}, "
          f"t: {loss_timestamps[-1]:.2f}s", flush=True)
end = time.perf_counter()
print(f"seconds per epoch: {(end - start) / max(args.num_epochs, 1):.4f}")

predicted, _ = predict_mean(test_x)
rmse = float(torch.sqrt(torch.mean((predicted - test_y) ** 2)))
loss_eval, _ = make_loss(len(test_x), 1e-4, 10_000)
with torch.no_grad():
    nll, _ = mll_lanczos(loss_eval, args.seed + 10_000, test_x, test_y)
print("NLL:", float(nll))
print("RMSE:", rmse)

directory = exp_util.matching_directory(os.path.abspath(__file__), "results/")
os.makedirs(directory, exist_ok=True)
path = f"{directory}{args.name}_{args.dataset}_s{args.seed}"
np.save(f"{path}_loss_timestamps.npy", np.asarray(loss_timestamps))
np.save(f"{path}_loss_curve.npy", np.asarray(loss_curve))
np.save(f"{path}_cg_errors.npy", np.asarray(cg_errors))
np.save(f"{path}_cg_numsteps.npy", np.asarray(cg_numsteps_all))
np.save(f"{path}_test_nlls.npy", np.asarray(float(nll)))
np.save(f"{path}_test_rmses.npy", np.asarray(rmse))
