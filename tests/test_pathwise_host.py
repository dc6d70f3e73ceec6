"""CPU-side checks of the pathwise GP posterior samples (no GPU): the two entry points are declared, mirrored and exported; bad
arguments are refused before any launch, by the C interface and by the Python layer; the same key gives the same features; the
frequency draws follow the spectral laws of the four kernels; and the dense restatement the GPU tests compare against
(tests/_pathwise_dense.py) represents the exact kernel at the Monte-Carlo rate."""

import ctypes
import math
import os
import re

import pytest
import torch

import _pathwise_dense as dense
from matfree_extensions import _lib, cg
from matfree_extensions.operators import RandomFeatures, RowShardedOp
from matfree_extensions.util import gp_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)  # a device pointer no kernel may touch: every call below must return before a launch
INVALID = -1
KERNELS = ["rbf", "matern12", "matern32", "matern52"]


def test_symbols_are_declared_mirrored_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "mfx.h")).read().split())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.get()
    for name in ("mfx_rff_apply", "mfx_rff_grad_x"):
        decl = re.search(r"int " + name + r"\(([^)]*)\);", header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(lib, name), name
        assert "`" + name + "`" in integration, name


def _apply(dtype=0, x=FAKE, ldx=3, n=5, d=3, omega=FAKE, phase=FAKE, m=4, ls=FAKE, ard=0, os_=FAKE, W=FAKE, ldw=4, S=2, out=FAKE,
           ldout=5):
    return _lib.get().mfx_rff_apply(dtype, x, ldx, n, d, omega, phase, m, ls, ard, os_, W, ldw, S, out, ldout, None)


def _grad(g=FAKE, ldg=5, dx=FAKE, lddx=3, **kw):
    a = dict(dtype=0, x=FAKE, ldx=3, n=5, d=3, omega=FAKE, phase=FAKE, m=4, ls=FAKE, ard=0, os_=FAKE, W=FAKE, ldw=4, S=2)
    a.update(kw)
    return _lib.get().mfx_rff_grad_x(a["dtype"], a["x"], a["ldx"], a["n"], a["d"], a["omega"], a["phase"], a["m"], a["ls"], a["ard"],
                                     a["os_"], a["W"], a["ldw"], a["S"], g, ldg, dx, lddx, None)


@pytest.mark.parametrize("bad, word", [
    (dict(dtype=7), "dtype"), (dict(x=None), "NULL"), (dict(omega=None), "NULL"), (dict(phase=None), "NULL"), (dict(ls=None), "NULL"),
    (dict(os_=None), "NULL"), (dict(W=None), "NULL"), (dict(n=0), "n = 0"), (dict(m=0), "m = 0"), (dict(S=0), "S = 0"),
    (dict(d=0), "d = 0"), (dict(d=1025, ldx=1025), "d = 1025"), (dict(ard=2), "ard"), (dict(ldx=2), "ldx"), (dict(ldw=3), "ldw"),
])
def test_c_interface_refuses_bad_arguments(bad, word):
    for call in (_apply, _grad):
        assert call(**bad) == INVALID
        assert word in _lib.get().mfx_last_error().decode()


def test_c_interface_refuses_bad_outputs():
    lib = _lib.get()
    for call, kw, word in ((_apply, dict(out=None), "out"), (_apply, dict(ldout=4), "ldout"), (_grad, dict(g=None), "g and dx"),
                           (_grad, dict(dx=None), "g and dx"), (_grad, dict(ldg=4), "ldg"), (_grad, dict(lddx=2), "lddx")):
        assert call(**kw) == INVALID and word in lib.mfx_last_error().decode()


def _features(kernel="rbf", key=5, d=3, m=7, S=2, dtype=torch.float64, **kw):
    return RandomFeatures(key, kernel=kernel, dim=d, num_features=m, num_samples=S, like=torch.zeros(1, dtype=dtype), **kw)


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_same_key_gives_the_same_features(kernel):
    a, b, c = _features(kernel, key=11), _features(kernel, key=11), _features(kernel, key=12)
    for name in ("omega", "phase", "weights"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert not torch.equal(getattr(a, name), getattr(c, name)), name
    assert a.omega.shape == (7, 3) and a.phase.shape == (7,) and a.weights.shape == (2, 7)
    assert 0 <= float(a.phase.min()) and float(a.phase.max()) < 2 * math.pi


def test_explicit_draws_are_taken_as_given():
    om, ph, w = torch.randn(7, 3, dtype=torch.float64), torch.rand(7, dtype=torch.float64), torch.randn(2, 7, dtype=torch.float64)
    f = _features(omega=om, phase=ph, weights=w)
    assert torch.equal(f.omega, om) and torch.equal(f.phase, ph) and torch.equal(f.weights, w)


def test_constructor_refuses_bad_shapes_and_kinds():
    with pytest.raises(ValueError, match="kernel"):
        _features("periodic")
    with pytest.raises(ValueError, match="dim"):
        _features(d=0)
    with pytest.raises(ValueError, match="dim"):
        _features(d=1025)
    with pytest.raises(ValueError, match="num_features"):
        _features(m=0)
    with pytest.raises(ValueError, match="num_features and num_samples"):
        _features(S=0)
    with pytest.raises(ValueError, match="omega"):
        _features(omega=torch.zeros(7, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="phase"):
        _features(phase=torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError, match="weights"):
        _features(weights=torch.zeros(3, 7, dtype=torch.float64))
    with pytest.raises(TypeError):
        RandomFeatures(1, kernel="rbf", dim=3, num_features=7, num_samples=2, like=torch.zeros(1, dtype=torch.float16))


def test_evaluate_refuses_cpu_tensors_bad_shapes_and_parameter_gradients():
    f = _features()
    one = torch.ones((), dtype=torch.float64)
    x = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(_lib.MfxError, match="no CPU fallback"):
        f.evaluate(x, one, one)
    for name, args in (("lengthscale", (x, one.clone().requires_grad_(), one)), ("outputscale", (x, one, one.clone().requires_grad_()))):
        with pytest.raises(ValueError, match=f"gradient with respect to {name} is refused"):
            f.evaluate(*args)
    for name in ("weights", "omega", "phase"):
        g = _features()
        getattr(g, name).requires_grad_()
        with pytest.raises(ValueError, match=f"gradient with respect to {name} is refused"):
            g.evaluate(x, one, one)


def test_pathwise_likelihood_refuses_row_sharded_operators_and_bad_counts():
    sharded = RowShardedOp.__new__(RowShardedOp)  # (a real one needs a process group; the refusal does not look at it)
    constrain = gp_util.constraint_greater_than(1e-4)
    solve = cg.cg_fixed_step(3)
    for A in (sharded, sharded.bind()):
        with pytest.raises(NotImplementedError, match="row-sharded"):
            gp_util.likelihood_condition_pathwise(A, solve, constrain=constrain, num_samples=2, num_features=4, key=1)
        with pytest.raises(NotImplementedError, match="row-sharded"):
            gp_util.likelihood_condition_pathwise_p(A, solve, precondition=None, constrain=constrain, num_samples=2, num_features=4,
                                                    key=1)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        gp_util.PathwisePosterior(sharded.bind(), solve, None, _features(), None, None)
    with pytest.raises(ValueError, match="num_samples"):
        gp_util.likelihood_condition_pathwise(gp_util.gram_matvec(), solve, constrain=constrain, num_samples=0, num_features=4, key=1)
    with pytest.raises(ValueError, match="num_features"):
        gp_util.likelihood_condition_pathwise(gp_util.gram_matvec(), solve, constrain=constrain, num_samples=2, num_features=0, key=1)


# ---- the frequency laws ------------------------------------------------------------------------------------------------------
def _cdf_abs(kernel, q):
    """P(|omega| <= q) for d = 1, q >= 0, = 2 F(q) - 1 with F the cdf of the symmetric law of omega."""
    if kernel == "rbf":  # N(0, 1)
        return math.erf(q / math.sqrt(2.0))
    if kernel == "matern12":  # Cauchy
        return 2.0 / math.pi * math.atan(q)
    if kernel == "matern32":  # Student t, 3 degrees of freedom
        u = q / math.sqrt(3.0)
        return 2.0 / math.pi * (u / (1 + u * u) + math.atan(u))
    u = q / math.sqrt(5.0)  # Student t, 5 degrees of freedom
    return 2.0 / math.pi * (u / (1 + u * u) * (1 + 2.0 / (3.0 * (1 + u * u))) + math.atan(u))


def _quantile_abs(kernel, p):
    lo, hi = 0.0, 1e6
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _cdf_abs(kernel, mid) < p else (lo, mid)
    return 0.5 * (lo + hi)


@pytest.mark.parametrize("kernel", KERNELS)
def test_frequency_draws_follow_the_spectral_law(kernel):
    """d = 1, N = 10^5 draws.  With s = |x - y| / l the kernels are sigma exp(-s^2 / 2), sigma exp(-s), sigma (1 + r) exp(-r) with
    r = sqrt(3) s and sigma (1 + r + r^2 / 3) exp(-r) with r = sqrt(5) s: Matern of smoothness nu with the distance scaled by sqrt(2 nu).
    By Bochner's theorem their normalised spectral densities are N(0, 1) for the RBF kernel and, for Matern-nu in one dimension,
    proportional to (1 + w^2 / (2 nu))^-(nu + 1/2): Student's t with 2 nu degrees of freedom -- Cauchy (nu = 1/2), t_3, t_5 -- which
    is z sqrt(2 nu / g) with z ~ N(0, 1) and g ~ chi^2_{2 nu}.  |omega| then has the cdf G(q) = 2 F(q) - 1 with
        F_normal(q) = (1 + erf(q / sqrt 2)) / 2,                  F_Cauchy(q) = 1/2 + atan(q) / pi,
        F_t3(q) = 1/2 + (u / (1 + u^2) + atan u) / pi,            u = q / sqrt 3,
        F_t5(q) = 1/2 + (u / (1 + u^2) (1 + 2 / (3 (1 + u^2))) + atan u) / pi,  u = q / sqrt 5,
    inverted by bisection for the quartiles.  An empirical p-quantile of N draws has the standard error sqrt(p (1 - p) / N) / G'(q_p)
    (G' by a central difference of the closed form); the bound is 5 of them."""
    N = 100_000
    f = RandomFeatures(2024, kernel=kernel, dim=1, num_features=N, num_samples=1, like=torch.zeros(1, dtype=torch.float64))
    draws = f.omega.abs().reshape(-1)
    for p in (0.25, 0.5, 0.75):
        q = _quantile_abs(kernel, p)
        h = 1e-5 * max(q, 1.0)
        density = (_cdf_abs(kernel, q + h) - _cdf_abs(kernel, q - h)) / (2 * h)
        stderr = math.sqrt(p * (1 - p) / N) / density
        got = float(torch.quantile(draws, p))
        print(f"{kernel} p={p}: analytic {q:.5f} empirical {got:.5f} |diff|/stderr {abs(got - q) / stderr:.2f}")
        assert abs(got - q) <= 5 * stderr, (kernel, p, got, q, stderr)
    # the phases are uniform on [0, 2 pi) and the weights standard normal: the same test on their quartiles
    for p in (0.25, 0.5, 0.75):
        stderr = math.sqrt(p * (1 - p) / N) * 2 * math.pi
        assert abs(float(torch.quantile(f.phase, p)) - 2 * math.pi * p) <= 5 * stderr


@pytest.mark.parametrize("kernel", KERNELS)
def test_dense_restatement_represents_the_exact_kernel(kernel):
    """c^2 sum_j cos(z_aj) cos(z_bj) is a mean of m independent terms 2 sigma cos cos, each bounded by 2 sigma with variance at most
    3 sigma^2 / 2, whose expectation is k(x_a, x_b): at m = 2 10^5 it sits within 5 sigma / sqrt(m) of the exact kernel."""
    m, d, sigma = 200_000, 2, 1.7
    f = RandomFeatures(7, kernel=kernel, dim=d, num_features=m, num_samples=1, like=torch.zeros(1, dtype=torch.float64))
    gen = torch.Generator().manual_seed(3)
    xa = torch.randn(6, d, dtype=torch.float64, generator=gen)
    xb = torch.randn(5, d, dtype=torch.float64, generator=gen)
    ls = torch.tensor([0.8, 1.3], dtype=torch.float64)
    s = torch.tensor(sigma, dtype=torch.float64)
    approx = dense.kernel_approx(xa, xb, f.omega, f.phase, ls, s)
    exact = dense.kernel_matrix(kernel, xa, xb, ls, s)
    err = float((approx - exact).abs().max())
    print(f"{kernel}: max |approx - exact| = {err:.3e}, bound {5 * sigma / math.sqrt(m):.3e}")
    assert err <= 5 * sigma / math.sqrt(m)


def test_draws_without_a_key_are_refused_with_a_clear_message():
    constrain = gp_util.constraint_greater_than(1e-4)
    solve = cg.cg_fixed_step(3)
    for key in (None, torch.zeros(2, 3)):
        with pytest.raises(ValueError, match="omega, phase, weights must be drawn"):
            _features(key=key)
        with pytest.raises(ValueError, match="phase must be drawn"):
            _features(key=key, omega=torch.zeros(7, 3, dtype=torch.float64), weights=torch.zeros(2, 7, dtype=torch.float64))
    with pytest.raises(ValueError, match="integer seed"):
        gp_util.likelihood_condition_pathwise(gp_util.gram_matvec(), solve, constrain=constrain, num_samples=2, num_features=4,
                                              key=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="missing: phase, eps"):
        gp_util.likelihood_condition_pathwise(gp_util.gram_matvec(), solve, constrain=constrain, num_samples=2, num_features=4, key=None,
                                              omega=torch.zeros(4, 3), weights=torch.zeros(2, 4))


def test_weights_are_made_row_contiguous_once_and_kept():
    w = torch.randn(7, 2, dtype=torch.float64).T  # (2, 7) with unit stride along the samples: not rows of unit stride
    f = _features(weights=w)
    assert f._weights.stride(1) == 1 and f._ldw >= 7 and torch.equal(f._weights, w)
    assert f._args(torch.zeros(4, 3, dtype=torch.float64), 3, torch.ones(1), torch.ones(1))[11].value == f._weights.data_ptr()
    wide = torch.randn(2, 12, dtype=torch.float64)
    g = _features(weights=wide[:, :7])
    assert g._ldw == 12 and g._weights.data_ptr() == wide.data_ptr()  # a row pitch is taken as it is, no copy
