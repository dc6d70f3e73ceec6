"""The three-term Lanczos recurrence (lanczos_forward_t) and its adjoint (lanczos_adjoint_t with k_lz_adj_dots, k_lz_adj_lambda,
k_lz_adj_xi, k_lz_adj_dvec) against the CPU oracle, element by element, at every launch geometry of tests/_lanczos_cases.py:
one wave and four, scalar and 16-byte loads, coarse and fine slices, one slice, two, 66 and 514 (the second load slot and the
second trip of reduce_partials_group<T, 64>), k = 1, dxs == NULL, dv == NULL and a misaligned dxs.

(a) through lanczos.tridiag(reortho="none") and autograd; (b) the adjoint driver alone on the oracle's forward pass rounded to the
kernel's type, so that a difference belongs to the adjoint kernels, with the adjoint states Lambda compared step by step.

The reference is the oracle in longdouble (dense cases) or float64 (the sparse cases, too large for longdouble).  The bounds are
lc.bounds: 32 x the oracle's own rounding error in the kernel's type, measured on the CPU (tests/test_lanczos_cases_host.py), relative
to the largest magnitude of the output per probe.  Outputs of the direct calls live between poisoned guard bands
(tests/_guarded_ws.py): a store past n in a ragged last slice lands in a band."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _lanczos_cases as lc
from _guarded_ws import GuardedWs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib, lanczos
    from matfree_extensions.operators import CsrOp, DenseOp

DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32]
NAME = {torch.float64: "float64", torch.float32: "float32"}
NP = {torch.float64: np.float64, torch.float32: np.float32}


def _dev(x, dtype):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=dtype, device=DEV)


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _reference_type(name):
    return "longdouble" if lc.case(name)[4] == "dense" else "float64"


def _operator(s, dtype):
    """(op, parameter on the device, select): select(gradient) gives the gradient entries in the layout of the reference"""
    if s.kind == "dense":
        rows = torch.as_tensor(s.rows, device=DEV)
        return DenseOp(), _dev(s.A, dtype), lambda g: _host(g[rows])
    op, vals, order = CsrOp.from_coo(s.row, s.col, s.vals, s.n, DEV)
    assert op.max_row_nnz == 5
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(order.numel())
    return op, vals.to(dtype), lambda g: _host(g)[inverse.numpy()]


def _check(failures, what, got, ref, bound, per_probe=True):
    """collects (what, error, bound) where max|got_b - ref_b| > bound * max|ref_b| for a probe b; prints every figure first"""
    err = lc.rel_err(got, ref, per_probe)
    print(f"    {what}: error {err:.3e}, bound {bound:.3e}")
    if not err <= bound:  # (also a NaN)
        failures.append((what, err, bound))


# ------------------------------------------------------------------------------------------------
# (a) lanczos.tridiag(reortho="none"), forward and autograd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("name", lc.NAMES, ids=lc.geometry_id)
def test_tridiag_none_and_its_gradient_against_the_oracle(name, dtype, monkeypatch):
    """xs, alpha, beta, q, b, dv and the parameter gradient, random cotangents on all five outputs, per probe.  The parameter
    gradient sums over all probes: it is compared where the oracle ran on all of them ("wg256-coarse": dv only).
    The workspace is exact-size and filled with 0xFF (NaN): row 0 of the forward's partial sums P1, which the single k_update of
    the three-term step relies on being zero, comes back as NaN wherever the driver does not zero it itself."""
    guard = GuardedWs(0xFF, busy=_lib._ws_busy)
    monkeypatch.setattr(_lib, "_take", guard.take)
    s = lc.case_inputs(name)
    k, probes = s.k, lc.reference_probes(name)
    ref, bound = lc.reference(name, _reference_type(name)), lc.bounds(name, NAME[dtype])
    op, param, select = _operator(s, dtype)
    param.requires_grad_(True)
    V = _dev(s.V, dtype).requires_grad_(True)
    (xs, (alpha, beta)), (q, b) = lanczos.tridiag(op, k, reortho="none")(V, param)
    dxs, dalpha, dbeta = _dev(s.dxs, dtype), _dev(s.dalpha, dtype), _dev(s.dbeta, dtype)
    cot = (dxs[:, :k], dalpha, dbeta[:, : k - 1], dxs[:, k], dbeta[:, k - 1])
    dv, dparam = torch.autograd.grad((xs, alpha, beta, q, b), (V, param), cot)
    torch.cuda.synchronize()
    guard.verify()
    failures = []
    _check(failures, "xs", _host(xs)[probes], ref["xs"][:, :k], bound["xs"])
    _check(failures, "q", _host(q)[probes], ref["xs"][:, k], bound["xs"])
    _check(failures, "alpha", _host(alpha)[probes], ref["alpha"], bound["alpha"])
    _check(failures, "beta and b", _host(torch.cat([beta, b[:, None]], dim=1))[probes], ref["beta"], bound["beta"])
    _check(failures, "dv", _host(dv)[probes], ref["dv"], bound["dv"])
    if len(probes) == s.p:
        _check(failures, "parameter gradient", select(dparam), ref["grad"], bound["grad"], per_probe=False)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------
# (b) mfx_lanczos_adjoint alone
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forward64(name):
    return lc.forward_pass(name, np.float64)


def _guarded(shape, dtype, zero=False):
    """(guard, tensor): `shape` elements between bands of 0xFF bytes (NaN as floats); the tensor itself starts as NaN or zero"""
    guard = GuardedWs(0xFF)
    t = guard.take(int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(), DEV).view(dtype).view(*shape)
    if zero:
        t.zero_()
    return guard, t


VARIANTS = ("dxs-null", "dv-null", "dxs-misaligned", "dalpha-only", "dbeta-only", "dxs-last-only")


def _adjoint_alone(name, dtype, variant, want_reference=True):
    """One direct call.  Returns (outputs on the device, reference): Lam (p, k, n), dv (p, n) or None, the parameter gradient
    in the reference's layout; the reference from lc.adjoint_pass on the same rounded forward pass and cotangents."""
    s = lc.case_inputs(name)
    n, k, p, probes = s.n, s.k, s.p, lc.reference_probes(name)
    fwd = tuple(f.astype(NP[dtype]) for f in _forward64(name))  # the oracle's forward, rounded to the kernel's type
    xs, alpha, beta = (_dev(f, dtype) for f in fwd)
    vnorm = _dev(np.linalg.norm(s.V, axis=1), dtype)
    cots = {"dxs": s.dxs, "dalpha": s.dalpha, "dbeta": s.dbeta}
    if variant in ("dalpha-only", "dbeta-only", "dxs-last-only"):
        cots = {key: np.zeros_like(val) for key, val in cots.items()}
        if variant == "dxs-last-only":
            cots["dxs"][:, k] = s.dxs[:, k]
        else:
            cots[variant[:-5]] = getattr(s, variant[:-5])
    elif variant == "dxs-null":
        cots["dxs"] = np.zeros_like(s.dxs)  # the reference: a zero basis cotangent
    ref_type = np.longdouble if s.kind == "dense" else np.float64
    ref = lc.adjoint_pass(name, ref_type, probes, forward=tuple(f[probes] for f in fwd), **cots) if want_reference else None

    if variant == "dxs-null":
        dxs = None
    elif variant == "dxs-misaligned":  # one element into its allocation: pick_vec must choose scalar loads
        dxs = torch.empty(p * (k + 1) * n + 1, dtype=dtype, device=DEV)[1:].view(p, k + 1, n)
        dxs.copy_(_dev(cots["dxs"], dtype))
        assert dxs.data_ptr() % 16 == dxs.element_size()
    else:
        dxs = _dev(cots["dxs"], dtype)
    dalpha, dbeta = _dev(cots["dalpha"], dtype), _dev(cots["dbeta"], dtype)

    op, param, select = _operator(s, dtype)
    desc = op.descriptor((param,), dtype, n)
    guards = {}
    guards["Lam"], Lam = _guarded((p, k, n), dtype)
    dv = None
    if variant != "dv-null":
        guards["dv"], dv = _guarded((p, n), dtype)
    guards["grad"], grad = _guarded(tuple(param.shape), dtype, zero=True)
    gs = _lib.OpGrads()
    if s.kind == "dense":
        gs.dense_a = grad.data_ptr()
    else:
        gs.val = grad.data_ptr()
    lib = _lib.get()
    guards["workspace"] = GuardedWs(0xFF)
    ws = guards["workspace"].take(int(lib.mfx_workspace_bytes(C.byref(desc), n, k, p)), DEV)
    _lib.check(lib.mfx_lanczos_adjoint(C.byref(desc), n, k, p, _lib.ptr(xs), _lib.ptr(alpha), _lib.ptr(beta), _lib.ptr(vnorm),
                                       _lib.ptr(dxs), _lib.ptr(dalpha), _lib.ptr(dbeta), _lib.ptr(dv), _lib.ptr(Lam), C.byref(gs),
                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    for guard in guards.values():
        guard.verify()
    return {"Lam": Lam, "dv": dv, "grad": grad, "select": select}, ref


def _check_adjoint(name, dtype, out, ref):
    s = lc.case_inputs(name)
    probes, bound = lc.reference_probes(name), lc.bounds(name, NAME[dtype])
    failures = []
    Lam = _host(out["Lam"])[probes]
    for j in range(s.k - 1, -1, -1):  # in the order the driver produces them: the first wrong step is the first reported
        _check(failures, f"lambda_{j}", Lam[:, j], ref["Lam"][:, j], bound["Lam"])
    if out["dv"] is not None:
        _check(failures, "dv", _host(out["dv"])[probes], ref["dv"], bound["dv"])
    if len(probes) == s.p:
        _check(failures, "parameter gradient", out["select"](out["grad"]), ref["grad"], bound["grad"], per_probe=False)
    assert not failures, failures


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("name", lc.NAMES, ids=lc.geometry_id)
def test_adjoint_states_step_by_step_on_the_oracle_forward(name, dtype):
    """Lam[:, j] against lambda_j for every j, then dv, then the parameter gradient, all cotangents random"""
    out, ref = _adjoint_alone(name, dtype, "all")
    _check_adjoint(name, dtype, out, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", lc.ADJOINT_VARIANT_CASES, ids=lc.geometry_id)
def test_adjoint_variants(name, variant, dtype):
    """dxs == NULL (reference: a zero basis cotangent); dv == NULL (Lam[:, 0] still written, Lam and the gradient bit for bit those
    of the call with dv); dxs one element into its allocation (scalar loads, same bounds); and one non-zero cotangent at a time --
    dalpha, dbeta, dxs[:, k] -- each isolating one term of mu, nu and xi"""
    out, ref = _adjoint_alone(name, dtype, variant)
    _check_adjoint(name, dtype, out, ref)
    if variant == "dv-null":
        with_dv, _ = _adjoint_alone(name, dtype, "all", want_reference=False)
        assert torch.equal(out["Lam"], with_dv["Lam"]) and torch.equal(out["grad"], with_dv["grad"])
