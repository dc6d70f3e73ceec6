"""Pathwise GP posterior samples on the GPU: the fused random-feature kernel (mfx_rff_apply), its VJP onto the points
(mfx_rff_grad_x) and Matheron's rule on top of them, against the dense torch restatement (tests/_pathwise_dense.py) on explicit draws.

Geometry under test (csrc/mfx_rff.hip): a workgroup owns 128 rows in fp32 and 64 in fp64; features are staged 32 at a time; samples
run in chunks of 16 or 64 (fp32) and 8 or 32 (fp64); the columns of x in chunks of 8 (d <= 8) or 16.  The shapes below sit at each of
those sizes minus one, exact, plus one, and at 1.

fp32 bounds come from the plain torch fp32 CPU evaluation of the same formula (4 x its error against fp64: the factor covers another
summation order) or 1e-6 c max_s sum_j |W_sj| (an absolute error of 1e-6 per cosine), whichever is larger; fp64 bounds are
1e-12 c max_s sum_j |W_sj|.  Neither comes from the code under test."""

import math

import pytest
import torch

import _pathwise_dense as dense
from matfree_extensions import cg, low_rank
from matfree_extensions.operators import RandomFeatures, RowShardedOp
from matfree_extensions.util import gp_util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KERNELS = ["rbf", "matern12", "matern32", "matern52"]
# the adaptive solvers stop on rms(r / (atol + rtol |x|)) <= 1 and pad their slices with zeros, so atol = 0 makes 0 / 0 there and the
# solve stops before its first step: "rtol 1e-12" is run with the smallest atol that avoids this, which changes no digit of the rule
TINY = 1e-300

N_EDGES = [1, 63, 64, 65, 127, 128, 129, 257]
M_EDGES = [1, 31, 32, 33, 100]
S_EDGES = [1, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]
SHAPES = ([(n, 33, 3) for n in N_EDGES] + [(65, m, 3) for m in M_EDGES] + [(65, 33, S) for S in S_EDGES]
          + [(1, 1, 1), (257, 100, 65), (129, 31, 17), (64, 32, 64), (128, 32, 16)])


def _draws(seed, n, d, m, S, dtype, ard, omega=None):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, dtype=dtype, generator=gen)
    omega = torch.randn(m, d, dtype=dtype, generator=gen) if omega is None else omega.to(dtype)
    phase = (2 * math.pi * torch.rand(m, dtype=torch.float64, generator=gen)).to(dtype)
    W = torch.randn(S, m, dtype=dtype, generator=gen)
    ls = (0.5 + torch.rand(d if ard else 1, dtype=torch.float64, generator=gen)).to(dtype)
    ls = ls if ard else ls.reshape(())
    s = torch.tensor(1.3, dtype=dtype)
    return x, omega, phase, W, ls, s


def _padded(t, pad):
    """the same values as rows of a wider tensor: a leading dimension that is no multiple of 4 elements"""
    wide = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    wide[:, : t.shape[1]] = t
    return wide[:, : t.shape[1]]


def _bound(ref64, cpu32, floor, dtype):
    if dtype == torch.float64:
        return 1e-12 * floor
    return max(4 * float((cpu32.double() - ref64).abs().max()), 1e-6 * floor)


def _forward_case(x, omega, phase, W, ls, s, padded):
    """-> (error, bound) of one mfx_rff_apply call"""
    dtype = x.dtype
    m = omega.shape[0]
    args64 = [t.double() for t in (x, omega, phase, W, ls, s)]
    ref = dense.features(*args64)
    cpu32 = dense.features(x, omega, phase, W, ls, s) if dtype == torch.float32 else None
    floor = math.sqrt(2 * float(s) / m) * float(W.double().abs().sum(1).max())
    xd, Wd = x.to(DEV), W.to(DEV)
    if padded:
        xd, Wd = _padded(xd, 3), _padded(Wd, 5)
    f = RandomFeatures(None, kernel="rbf", dim=x.shape[1], num_features=m, num_samples=W.shape[0], like=xd, omega=omega.to(DEV),
                       phase=phase.to(DEV), weights=Wd)
    got = f.evaluate(xd, ls.to(DEV), s.to(DEV))
    assert got.shape == ref.shape and got.dtype == dtype
    return float((got.double().cpu() - ref).abs().max()), _bound(ref, cpu32, floor, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("ard", [False, True], ids=["scalar", "ard"])
@pytest.mark.parametrize("d", [1, 2, 8, 9, 16, 17, 33])
def test_feature_kernel_at_every_tile_edge(d, ard, dtype):
    worst = 0.0
    for k, (n, m, S) in enumerate(SHAPES):
        draws = _draws(1000 * d + k, n, d, m, S, dtype, ard)
        for padded in (False, True):
            err, bound = _forward_case(*draws, padded)
            worst = max(worst, err / bound)
            assert err <= bound, (n, m, S, d, ard, padded, err, bound)
    print(f"d={d} ard={ard} {dtype}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_large_phases_are_range_reduced(dtype):
    """Matern-1/2 (Cauchy) frequencies from a fixed key: phases beyond 10^3 radians, where a cosine without range reduction fails."""
    n, d, m, S = 257, 3, 2048, 5
    drawn = RandomFeatures(4242, kernel="matern12", dim=d, num_features=m, num_samples=S, like=torch.zeros(1, dtype=torch.float64))
    x, omega, phase, W, ls, s = _draws(77, n, d, m, S, dtype, True, omega=drawn.omega)
    big = float(dense.phases(x.double(), omega.double(), phase.double(), ls.double()).abs().max())
    assert big >= 1e3, big
    err, bound = _forward_case(x, omega, phase, W, ls, s, False)
    print(f"{dtype}: max |phase| = {big:.3e}, error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def _grad_case(n, d, m, S, dtype, ard, seed):
    x, omega, phase, W, ls, s = _draws(seed, n, d, m, S, dtype, ard)
    gen = torch.Generator().manual_seed(seed + 1)
    g = torch.randn(S, n, dtype=dtype, generator=gen)

    def dense_grad(dt):
        xx = x.to(dt).requires_grad_()
        out = dense.features(xx, omega.to(dt), phase.to(dt), W.to(dt), ls.to(dt), s.to(dt))
        return torch.autograd.grad((out * g.to(dt)).sum(), xx)[0]

    ref = dense_grad(torch.float64)
    f = RandomFeatures(None, kernel="rbf", dim=d, num_features=m, num_samples=S, like=x.to(DEV), omega=omega.to(DEV), phase=phase.to(DEV),
                       weights=W.to(DEV))
    grads = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_()
        out = f.evaluate(xd, ls.to(DEV), s.to(DEV))
        grads.append(torch.autograd.grad(out, xd, g.to(DEV))[0])
    assert torch.equal(grads[0], grads[1])  # bit-reproducible
    return grads[0].double().cpu(), ref, dense_grad(torch.float32) if dtype == torch.float32 else None, (omega, W, ls, s, g)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("d", [1, 9])
@pytest.mark.parametrize("n", [1, 65])
def test_grad_x_fp64_matches_autograd_through_the_dense_restatement(n, d, S):
    got, ref, _, _ = _grad_case(n, d, 33, S, torch.float64, True, 31 * n + 7 * d + S)
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= 1e-9 * scale


@pytest.mark.parametrize("n, d, m, S", [(1, 1, 33, 1), (65, 9, 33, 3), (129, 17, 100, 17), (257, 8, 31, 65), (128, 33, 32, 64)])
def test_grad_x_fp32_within_the_cpu_fp32_error(n, d, m, S):
    """Bound as for the forward: 4 x the error of the torch fp32 CPU gradient, or an absolute error of 1e-6 per sine:
    1e-6 c max_{i,t} sum_s sum_j |g_si W_sj omega_jt| / l_t."""
    got, ref, cpu32, (omega, W, ls, s, g) = _grad_case(n, d, m, S, torch.float32, True, 5 * n + d)
    c = math.sqrt(2 * float(s) / m)
    floor = c * float(((g.double().abs().T @ W.double().abs()) @ omega.double().abs() / ls.double()).max())
    bound = max(4 * float((cpu32.double() - ref).abs().max()), 1e-6 * floor)
    err = float((got - ref).abs().max())
    print(f"n={n} d={d} m={m} S={S}: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ---- Matheron's rule ---------------------------------------------------------------------------------------------------------
def _gp(kind, dtype, n, d, seed, noise=0.1):
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, dtype=dtype, generator=gen)
    y = torch.sin(X.sum(1)) + 0.1 * torch.randn(n, dtype=dtype, generator=gen)
    inv_softplus = lambda v: math.log(math.expm1(v))
    raw = {"ls": torch.tensor(inv_softplus(0.9), dtype=dtype), "s": torch.tensor(inv_softplus(1.4), dtype=dtype),
           "noise": torch.tensor(inv_softplus(noise), dtype=dtype), "mean": torch.tensor(0.3, dtype=dtype)}
    return X, y, raw


def _posterior(kind, likelihood, X, y, raw):
    kernels = {"rbf": gp_util.kernel_scaled_rbf, "matern12": gp_util.kernel_scaled_matern_12, "matern32": gp_util.kernel_scaled_matern_32,
               "matern52": gp_util.kernel_scaled_matern_52}
    kernel, _ = kernels[kind](shape_in=(X.shape[1],), shape_out=())
    mean, _ = gp_util.mean_constant(shape_out=())
    post = gp_util.target_posterior(gp_util.model_gp(mean, kernel), likelihood[0])
    predict, _ = post(X.to(DEV), y.to(DEV), {"constant_value": raw["mean"].to(DEV)},
                      {"raw_lengthscale": raw["ls"].to(DEV), "raw_outputscale": raw["s"].to(DEV)}, {"raw_noise": raw["noise"].to(DEV)})
    return predict


@pytest.mark.parametrize("preconditioned", [False, True], ids=["cg", "pcg"])
@pytest.mark.parametrize("kind", KERNELS)
def test_matheron_rule_matches_the_dense_restatement(kind, preconditioned):
    n, d, S, m, noise = 200, 3, 5, 64, 0.1
    dt = torch.float64
    X, y, raw = _gp(kind, dt, n, d, 17, noise)
    drawn = RandomFeatures(99, kernel=kind, dim=d, num_features=m, num_samples=S, like=X)
    gen = torch.Generator().manual_seed(5)
    eps = math.sqrt(noise) * torch.randn(S, n, dtype=dt, generator=gen)
    xs = torch.randn(37, d, dtype=dt, generator=gen)
    xs2 = torch.cat([xs[30:33], torch.randn(8, d, dtype=dt, generator=gen)])
    constrain = gp_util.constraint_greater_than(0.0)
    explicit = dict(omega=drawn.omega.to(DEV), phase=drawn.phase.to(DEV), weights=drawn.weights.to(DEV), eps=eps.to(DEV))
    common = dict(constrain=constrain, num_samples=S, num_features=m, key=None, **explicit)
    if preconditioned:
        like = gp_util.likelihood_condition_pathwise_p(gp_util.gram_matvec(), cg.pcg_adaptive(atol=TINY, rtol=1e-12, maxiter=400),
                                                       precondition=low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=20)),
                                                       **common)
    else:
        like = gp_util.likelihood_condition_pathwise(gp_util.gram_matvec(), cg.cg_adaptive(atol=TINY, rtol=1e-12, maxiter=400), **common)
    paths, info = _posterior(kind, like, X, y, raw)(xs.to(DEV))
    assert "solve" in info

    sp = torch.nn.functional.softplus
    hyper = (sp(raw["ls"]), sp(raw["s"]), sp(raw["noise"]))

    def dense_paths(points):
        return dense.matheron(kind, X, y, raw["mean"], points, drawn.omega, drawn.phase, drawn.weights, eps, *hyper)

    xg = xs.to(DEV).requires_grad_()
    got = paths(xg)
    ref = dense_paths(xs)
    assert got.shape == (S, 37)
    scale = float(ref.abs().max())
    err = float((got.detach().cpu() - ref).abs().max())
    print(f"{kind} preconditioned={preconditioned}: error {err:.3e}, bound {1e-8 * scale:.3e}")
    assert err <= 1e-8 * scale
    # the same functions at a second point set: rows of the shared points agree
    got2 = paths(xs2.to(DEV))
    assert got2.shape == (S, 11)
    assert float((got2[:, :3] - got.detach()[:, 30:33]).abs().max()) <= 1e-12 * scale
    assert float((got2.cpu() - dense_paths(xs2)).abs().max()) <= 1e-8 * scale
    # the gradient with respect to the points
    (gx,) = torch.autograd.grad(got.sum(), xg)
    xr = xs.clone().requires_grad_()
    (gref,) = torch.autograd.grad(dense_paths(xr).sum(), xr)
    assert float((gx.cpu() - gref).abs().max()) <= 1e-7 * float(gref.abs().max())


MOMENTS_KEY = 20240
NEAR_POINTS = 12  # test points whose exact posterior variance is below sigma_f / 4 (dense restatement)


def _moments_setup():
    n, d, S, m = 256, 2, 512, 2048
    dt = torch.float32
    X, y, raw = _gp("rbf", dt, n, d, 23, 0.1)
    drawn = RandomFeatures(MOMENTS_KEY, kernel="rbf", dim=d, num_features=m, num_samples=S, like=X)  # drawn on the CPU: the same on any device
    gen = torch.Generator().manual_seed(MOMENTS_KEY + 1)
    eps = math.sqrt(0.1) * torch.randn(S, n, dtype=dt, generator=gen)
    xs = 1.5 * torch.randn(16, d, dtype=dt, generator=gen)
    return X, y, raw, drawn, eps, xs, (n, d, S, m)


def _moment_bounds(var, S, m, sigma):
    feature = 3 * sigma / math.sqrt(m)
    return 5 * torch.sqrt(var / S) + feature, 5 * var * math.sqrt(2.0 / (S - 1)) + feature


def test_moments_of_the_paths_match_the_exact_posterior():
    """The sample mean and variance over S = 512 paths against likelihood_condition and likelihood_condition_var: 5 standard errors
    (5 sqrt(var / S) for the mean, 5 var sqrt(2 / (S - 1)) for the variance) plus 3 sigma_f / sqrt(m) for the feature approximation.
    With key 20240 the dense fp64 restatement on the same draws (a CPU computation, not this run) sits at most 0.161 of the bound
    (mean) and 0.335 (variance) over the 16 points: inside the half that the choice of the key has to leave.

    The solves must really run: every right-hand side takes at least one CG step, and at 12 of the 16 test points the exact
    posterior variance is below sigma_f / 4 (0.005 to 0.33 against sigma_f = 1.4 in the dense restatement), so paths
    that lack the K(x*, X) v_s update -- prior draws, whose variance is sigma_f everywhere -- miss the variance bound there."""
    X, y, raw, drawn, eps, xs, (n, d, S, m) = _moments_setup()
    constrain = gp_util.constraint_greater_than(0.0)
    solve = cg.cg_adaptive(atol=1e-6, rtol=0.0, maxiter=1000, miniter=1)  # (atol = 0: see TINY above)
    like = gp_util.likelihood_condition_pathwise(gp_util.gram_matvec(precision="fp32"), solve, constrain=constrain, num_samples=S,
                                                 num_features=m, key=None, omega=drawn.omega.to(DEV), phase=drawn.phase.to(DEV),
                                                 weights=drawn.weights.to(DEV), eps=eps.to(DEV))
    paths, info = _posterior("rbf", like, X, y, raw)(xs.to(DEV))
    assert info["solve"]["num_steps"].shape == (S,) and int(info["solve"]["num_steps"].min()) > 0
    f = paths(xs.to(DEV)).double().cpu()
    exact = gp_util.likelihood_condition_var(gp_util.gram_matvec(precision="fp32"), solve, constrain=constrain)
    (mu, var), einfo = _posterior("rbf", exact, X, y, raw)(xs.to(DEV))
    assert int(einfo["solve"]["num_steps"].min()) > 0 and int(einfo["variance_solve"]["num_steps"].min()) > 0
    mu, var = mu.double().cpu(), var.double().cpu()
    sigma = float(torch.nn.functional.softplus(raw["s"]))
    informed = var < sigma / 4
    assert int(informed.sum()) >= NEAR_POINTS, var
    assert bool(((f.var(0) - sigma).abs()[informed] > 5 * sigma * math.sqrt(2.0 / (S - 1)) + 3 * sigma / math.sqrt(m)).all())  # not prior draws
    bmean, bvar = _moment_bounds(var, S, m, sigma)
    rmean, rvar = (f.mean(0) - mu).abs() / bmean, (f.var(0) - var).abs() / bvar
    print(f"mean: worst error / bound {float(rmean.max()):.3f}; variance: {float(rvar.max()):.3f}")
    assert bool((rmean <= 1).all()) and bool((rvar <= 1).all())


def test_bad_calls_are_refused():
    sharded = RowShardedOp.__new__(RowShardedOp)  # (a real one needs a process group; the refusal does not look at it)
    constrain = gp_util.constraint_greater_than(0.0)
    solve = cg.cg_fixed_step(3)
    with pytest.raises(NotImplementedError, match="not available on row-sharded operators"):
        gp_util.likelihood_condition_pathwise(sharded, solve, constrain=constrain, num_samples=2, num_features=8, key=1)
    X, y, raw = _gp("rbf", torch.float32, 40, 2, 3)
    raw["ls"] = raw["ls"].to(DEV).requires_grad_()
    like = gp_util.likelihood_condition_pathwise(gp_util.gram_matvec(), solve, constrain=constrain, num_samples=2, num_features=8, key=1)
    with pytest.raises(ValueError, match="gradient with respect to lengthscale is refused"):
        _posterior("rbf", like, X, y, raw)(None)
    f = RandomFeatures(1, kernel="rbf", dim=2, num_features=8, num_samples=2, like=X.to(DEV))
    with pytest.raises(ValueError, match=r"must be \(n >= 1, 2\)"):
        f.evaluate(torch.zeros(4, 3, device=DEV), torch.ones((), device=DEV), torch.ones((), device=DEV))
    with pytest.raises(TypeError, match="dtype of the features"):
        f.evaluate(torch.zeros(4, 2, device=DEV, dtype=torch.float64), torch.ones((), device=DEV), torch.ones((), device=DEV))
