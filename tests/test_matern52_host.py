"""Matern-5/2 on the host side (no GPU): the plain-torch kernel of gp_util against the closed form, the value at distance 0,
the C-ABI constant, the operator descriptor.

    s = sum_c ((x_c - y_c) / l_c)^2 clamped at 0,   r = sqrt(5 s + eps),   k = sigma (1 + r + r^2 / 3) exp(-r)
    dk/dl_c = sigma w (x_c - y_c)^2 / l_c^3 with w = (5 / 3) (1 + r) exp(-r)     (the convention of csrc/mfx_kernel_fn.h)
"""

import math
import os
import re

import pytest
import torch

from matfree_extensions import _lib
from matfree_extensions.operators import RbfGramOp, _kappa0
from matfree_extensions.util import gp_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def closed_form(x, y, ls, s, eps):
    dist = sum(((float(a) - float(b)) / float(l)) ** 2 for a, b, l in zip(x, y, ls))
    r = math.sqrt(5.0 * dist + eps)
    return s * (1.0 + r + r * r / 3.0) * math.exp(-r), (5.0 / 3.0) * (1.0 + r) * math.exp(-r)


def test_kernel_scaled_matern_52_matches_the_closed_form_in_fp64():
    d = 3
    parametrize, like = gp_util.kernel_scaled_matern_52(shape_in=(d,), shape_out=())
    assert like["raw_lengthscale"].shape == (d,) and like["raw_outputscale"].shape == ()
    g = torch.Generator().manual_seed(0)
    raw_l = torch.randn(d, generator=g, dtype=torch.float64)
    raw_s = torch.tensor(0.3, dtype=torch.float64)
    k = parametrize(raw_lengthscale=raw_l, raw_outputscale=raw_s)
    assert k.native[0] == "matern52" and k.native[1] is raw_l and k.native[2] is raw_s
    ls, s = torch.nn.functional.softplus(raw_l), float(torch.nn.functional.softplus(raw_s))
    eps = float(torch.finfo(torch.float64).eps)
    for _ in range(8):
        x, y = torch.randn(d, generator=g, dtype=torch.float64), torch.randn(d, generator=g, dtype=torch.float64)
        want, _ = closed_form(x, y, ls, s, eps)
        assert abs(float(k(x, y)) - want) <= 1e-14 * s
        assert float(k(x, y)) == float(k(y, x))
    x = torch.randn(d, generator=g, dtype=torch.float64)
    r0 = math.sqrt(eps)
    assert abs(float(k(x, x)) - s * (1.0 + r0 + r0 * r0 / 3.0) * math.exp(-r0)) <= 1e-15 * s  # x = y: the clamped side, r = sqrt(eps)


def test_lengthscale_gradient_is_the_weight_of_the_device_code():
    d = 4
    parametrize, _ = gp_util.kernel_scaled_matern_52(shape_in=(d,), shape_out=())
    g = torch.Generator().manual_seed(1)
    eps = float(torch.finfo(torch.float64).eps)
    for _ in range(6):
        raw_l = torch.randn(d, generator=g, dtype=torch.float64).requires_grad_(True)
        raw_s = torch.randn((), generator=g, dtype=torch.float64)
        x, y = torch.randn(d, generator=g, dtype=torch.float64), torch.randn(d, generator=g, dtype=torch.float64)
        ls = torch.nn.functional.softplus(raw_l).detach()
        (gl,) = torch.autograd.grad(parametrize(raw_lengthscale=raw_l, raw_outputscale=raw_s)(x, y), raw_l)
        gl = gl / torch.sigmoid(raw_l.detach())  # d softplus: back from the raw parameter to the lengthscale
        s = float(torch.nn.functional.softplus(raw_s))
        _, w = closed_form(x, y, ls, s, eps)
        want = s * w * (x - y) ** 2 / ls ** 3
        assert float((gl - want).abs().max()) <= 1e-11 * s  # 2e-12 measured
    # no kink at 0: the weight at x = y is (5 / 3) (1 + sqrt(eps)) exp(-sqrt(eps)), times a zero difference
    raw_l = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    x = torch.randn(d, generator=g, dtype=torch.float64)
    (gl,) = torch.autograd.grad(parametrize(raw_lengthscale=raw_l, raw_outputscale=torch.tensor(0.0, dtype=torch.float64))(x, x), raw_l)
    assert torch.equal(gl, torch.zeros_like(gl))


def test_shape_errors_as_for_the_other_kernels():
    parametrize, _ = gp_util.kernel_scaled_matern_52(shape_in=(3,), shape_out=())
    k = parametrize(raw_lengthscale=torch.zeros(3), raw_outputscale=torch.zeros(()))
    other, _ = gp_util.kernel_scaled_matern_32(shape_in=(3,), shape_out=())
    k32 = other(raw_lengthscale=torch.zeros(3), raw_outputscale=torch.zeros(()))
    for x, y in ((torch.zeros(3), torch.zeros(4)), (torch.zeros(4), torch.zeros(4)), (torch.zeros(3, 1), torch.zeros(3, 1))):
        with pytest.raises(ValueError) as e52:
            k(x, y)
        with pytest.raises(ValueError) as e32:
            k32(x, y)
        assert str(e52.value) == str(e32.value)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_kappa0_is_the_formula_at_distance_zero(dtype):
    r0 = math.sqrt(torch.finfo(dtype).eps)
    want = (1.0 + r0 + r0 * r0 / 3.0) * math.exp(-r0)
    assert _kappa0("matern52", dtype) == pytest.approx(want, rel=0, abs=1e-16)
    assert 0.0 < 1.0 - _kappa0("matern52", dtype) < 1e-7  # 1 - eps / 6: 2.0e-8 with the fp32 eps
    assert _kappa0("matern52", dtype) >= _kappa0("matern32", dtype) > _kappa0("matern12", dtype)  # 1 - eps/6, 1 - eps/2, 1 - sqrt(eps)
    parametrize, _ = gp_util.kernel_scaled_matern_52(shape_in=(2,), shape_out=())
    x = torch.tensor([0.3, -1.2], dtype=dtype)
    k = parametrize(raw_lengthscale=torch.zeros(2, dtype=dtype), raw_outputscale=torch.zeros((), dtype=dtype))
    s = float(torch.nn.functional.softplus(torch.zeros((), dtype=dtype)))
    assert float(k(x, x)) == pytest.approx(s * _kappa0("matern52", dtype), rel=2 * torch.finfo(dtype).eps)


def test_header_and_python_agree_on_the_constant():
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    values = dict(re.findall(r"(MFX_KERNEL_[A-Z0-9]+) = (\d+)", header))
    assert values == {"MFX_KERNEL_RBF": "0", "MFX_KERNEL_MATERN12": "1", "MFX_KERNEL_MATERN32": "2", "MFX_KERNEL_MATERN52": "3"}
    assert (_lib.KERNEL_RBF, _lib.KERNEL_MATERN12, _lib.KERNEL_MATERN32, _lib.KERNEL_MATERN52) == (0, 1, 2, 3)
    assert re.search(r"#define MFX_VERSION 201\b", header)  # additive: no version bump
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.get().mfx_version() == 201


def test_operator_takes_the_new_family_and_refuses_unknown_ones():
    X = torch.randn(10, 3)
    op = RbfGramOp(X, kernel="matern52")
    assert op.kernel == "matern52" and RbfGramOp._KERNELS["matern52"] == 3
    params = (torch.zeros(3), torch.zeros(()), torch.zeros(()))
    desc = op.descriptor(op.constrain(*params), torch.float32, 10)
    assert desc.kernel_fn == 3 and desc.kind == _lib.OP_RBF and desc.d == 3
    assert gp_util.gram_operator(X, kernel="matern52").kernel == "matern52"
    with pytest.raises(ValueError, match="matern52"):
        RbfGramOp(X, kernel="matern72")


def test_native_cov_reads_the_family_from_the_kernel():
    with pytest.raises(TypeError, match="kernel_scaled_matern_52"):
        gp_util._native_cov(gp_util.gram_matvec(), torch.zeros(4, 2), lambda x, y: x @ y, gp_util.constraint_greater_than(0.0), torch.zeros(()))
    parametrize, _ = gp_util.kernel_scaled_matern_52(shape_in=(2,), shape_out=())
    k = parametrize(raw_lengthscale=torch.zeros(2), raw_outputscale=torch.zeros(()))
    bound = gp_util._native_cov(gp_util.gram_matvec(), torch.zeros(4, 2), k, gp_util.constraint_greater_than(1e-3), torch.zeros(()))
    assert bound.op.kernel == "matern52"
