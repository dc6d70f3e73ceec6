"""Cases, references, launch geometry and error bounds for the three-term Lanczos recurrence (lanczos_forward_t) and its adjoint
(lanczos_adjoint_t: k_lz_adj_dots, k_lz_adj_lambda, k_lz_adj_xi, k_lz_adj_dvec) -- plain numpy, no GPU.
tests/test_lanczos_cases_host.py checks this file against itself and the oracle on the CPU; tests/test_gpu_lanczos_kernels.py
compares the HIP kernels with it.

Every input (matrix, start vectors, cotangents) is rounded to float32 once, so it is exactly representable in float32, float64 and
longdouble alike: one longdouble reference serves the kernels of both types, and no type sees another operator than the others.

The bounds of DENSE_BOUNDS do not come from the kernels.  They are 32 times the error of the numpy oracle run in the same floating-point
type against the oracle run in longdouble (u = 2^-64), measured on the CPU: `python tests/_lanczos_cases.py` prints the table,
tests/test_lanczos_cases_host.py re-measures it and asserts that every stored bound lies within [16, 64] times the measurement.
The factor 32 covers the different order of summation (kernels: per thread, wave tree, slices; numpy: pairwise or BLAS blocks):
the two errors are of one size, not equal."""

import functools
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _ragged_csr as rc
from oracle import slq_oracle as orc

OUTPUTS = ("xs", "alpha", "beta", "Lam", "dv", "grad")  # xs holds the k + 1 vectors (basis and remainder), beta all k lengths
DENSE_MAX_N = 4200
SPARSE_OFFSETS = (1, 37)

CASES = (
    # name                   n        p    k  operator
    ("one-wave-scalar", 1531, 1, 9, "dense"),        # wg 64, VEC 1, three slices of 512, ragged tail
    ("one-wave-vector", 1536, 1, 9, "dense"),        # wg 64, 16-byte loads
    ("wg256-scalar", 1027, 16, 4, "dense"),          # wg 256, VEC 1, one slice
    ("wg256-vector", 1028, 16, 4, "dense"),          # forward: fine slices of 1024 / 512; adjoint: EPT 8
    ("wg256-coarse", 1028, 128, 4, "dense"),         # 128 workgroups: the forward stays coarse as well
    ("two-slices-scalar", 3075, 16, 4, "dense"),     # ragged second slice of 2048
    ("two-slices-vector", 3076, 16, 4, "dense"),     # ragged second slice; forward: 4 / 7 fine slices
    ("depth-one", 1028, 3, 1, "dense"),              # k = 1: lam_plus is always null
    ("many-slices-scalar", 133121, 1, 4, "sparse"),  # 66 slices: more partial sums than lanes
    ("many-slices-vector", 133124, 1, 4, "sparse"),  # forward: 131 (fp32) / 261 (fp64) fine slices
    ("second-trip", 1050628, 1, 2, "sparse"),        # 514 slices of 2048: second trip of the partial-sum loop
)
NAMES = tuple(c[0] for c in CASES)
DENSE_NAMES = tuple(c[0] for c in CASES if c[4] == "dense")
SPARSE_NAMES = tuple(c[0] for c in CASES if c[4] == "sparse")
ADJOINT_VARIANT_CASES = ("one-wave-scalar", "wg256-vector", "two-slices-vector")


def case(name):
    """(name, n, p, k, operator kind)"""
    return next(c for c in CASES if c[0] == name)


# ------------------------------------------------------------------------------------------------
# launch geometry (csrc/mfx_vec.h: pick_wg, pick_vec, Ctx, Ctx::fine -- restated once, in tests/_ragged_csr.py)
# ------------------------------------------------------------------------------------------------
def lanczos_geometry(n, p, dtype_name, aligned=True, adjoint=False):
    """(wg, VEC, EPT, nblk) of the vector kernels of lanczos_forward_t, or of lanczos_adjoint_t, which never calls Ctx::fine():
    its four kernels are compiled for kEpt elements per thread only.  nblk is the number of slices (partial sums per dot)."""
    wg, vec, ept = rc.csr_step_geometry(n, p, dtype_name, aligned)
    if adjoint:
        ept = rc.K_EPT
    return wg, vec, ept, -(-n // (wg * ept))


def geometry_id(name):
    _, n, p, k, _ = case(name)
    parts = [f"{name}-n{n}-p{p}-k{k}"]
    for dt, short in (("float32", "f32"), ("float64", "f64")):
        for adjoint in (False, True):
            wg, vec, ept, nblk = lanczos_geometry(n, p, dt, adjoint=adjoint)
            parts.append(f"{short}{'adj' if adjoint else 'fwd'}:wg{wg}.vec{vec}.ept{ept}.nblk{nblk}")
    return "-".join(parts)


def takes_fused_csr_step(name):
    """csr_fusable (csrc/mfx_krylov.hip): a CSR operator, not row-sharded, with values, whose longest row (and column) has at
    most 64 entries -- whatever the slicing.  The sparse operator's longest row has 5."""
    return case(name)[4] == "sparse" and 2 * len(SPARSE_OFFSETS) + 1 <= 64


# ------------------------------------------------------------------------------------------------
# operators and inputs
# ------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def dense_matrix(n, rng):
    """A = 2 I + 0.25 (B + B^T) / sqrt(n), B standard normal: symmetric, spectrum within about 2 +- 0.71"""
    B = rng.standard_normal((n, n))
    return _f32(2.0 * np.eye(n) + 0.25 * (B + B.T) / np.sqrt(n))  # rounding keeps the symmetry: both halves round alike


def sparse_coo(n, rng):
    """COO (row, col, vals), sorted by row then column: diagonal 2, symmetric uniform [-0.2, 0.2] entries at the offsets +-1 and
    +-37.  Rows of at most 5 entries; Gershgorin: spectrum within 2 +- 0.8."""
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [np.full(n, 2.0)]
    for d in SPARSE_OFFSETS:
        i = np.arange(n - d)
        w = rng.uniform(-0.2, 0.2, n - d)
        rows += [i, i + d]
        cols += [i + d, i]
        vals += [w, w]
    row, col, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((col, row))
    return row[order], col[order], _f32(vals[order])


def grad_rows(n):
    """The rows of the dense parameter gradient that are compared (all columns of each): the first and last two, the rows around
    every 512-element boundary and 16 spread evenly.  The gradient sweep k_dense_grad is pinned entry by entry in
    tests/test_gpu_operator_kernels.py; here it only carries the adjoint states, and a longdouble n x n outer product per probe
    would cost more than the recurrence itself."""
    rows = {0, 1, n - 2, n - 1} | {int(r) for r in np.linspace(0, n - 1, 16)}
    for edge in range(512, n, 512):
        rows |= {edge - 1, edge}
    return np.array(sorted(rows), dtype=np.int64)


class DenseRowsOp(orc.DenseOp):
    """orc.DenseOp whose parameter gradient sum_b cot_b v_b^T is formed on the rows grad_rows(n) only"""

    def __init__(self, rows):
        self.rows = rows

    def param_vjp(self, v, cot, A):
        return (np.atleast_2d(cot)[:, self.rows].T @ np.atleast_2d(v),)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """The operator, the p start vectors and random cotangents on all five outputs, deterministic, float64 arrays of
    float32-representable values.  Cotangents in the driver's layout: dxs (p, k + 1, n), dalpha (p, k), dbeta (p, k)."""
    idx = NAMES.index(name)
    _, n, p, k, kind = case(name)
    rng = np.random.default_rng(4100 + idx)
    s = types.SimpleNamespace(name=name, n=n, p=p, k=k, kind=kind)
    if kind == "dense":
        s.A = dense_matrix(n, rng)
        s.rows = grad_rows(n)
    else:
        s.row, s.col, s.vals = sparse_coo(n, rng)
    s.V = _f32(rng.standard_normal((p, n)))
    s.dxs = _f32(rng.standard_normal((p, k + 1, n)))
    s.dalpha = _f32(rng.standard_normal((p, k)))
    s.dbeta = _f32(rng.standard_normal((p, k)))
    return s


def oracle_operator(s, dtype):
    """(op, params) of the oracle in the numpy float type dtype"""
    if s.kind == "dense":
        return DenseRowsOp(s.rows), (s.A.astype(dtype),)
    return orc.CooOp(s.row, s.col, s.n), (s.vals.astype(dtype),)


def cotangent(dxs, dalpha, dbeta):
    """one probe's cotangents in the pytree of orc.tridiag_none's outputs"""
    k = dalpha.shape[0]
    return (dxs[:k], (dalpha, dbeta[: k - 1])), (dxs[k], dbeta[k - 1])


def reference_probes(name):
    return rc.oracle_probes(case(name)[2])


# ------------------------------------------------------------------------------------------------
# the step-wise adjoint reference
# ------------------------------------------------------------------------------------------------
def tridiag_none_vjp_states(op, k, v, params, cot, forward=None):
    """orc.tridiag_none_vjp restated, in the float type of its arguments, returning (dvec, dparams, lams (k, n), munu (k, 2)):
    also the adjoint states lambda_j and the scalars (mu_j, nu_j), indexed by the step j they belong to.
    forward = (xs (k + 1, n), alpha (k,), beta (k,)): run the adjoint recurrence on this forward pass instead of the oracle's own
    (the direct calls of the adjoint driver hand it a forward pass rounded to the kernel's type)."""
    (dxs_, (da, db_)), (dx_last, db_last) = cot
    if forward is None:
        (xs_, (a, b_)), (x_last, b_last) = orc.tridiag_none(op, k, v, *params)
        xs = np.concatenate([xs_, x_last[None]])
        b = np.concatenate([b_, [b_last]])
    else:
        xs, a, b = forward
    dxs = np.concatenate([dxs_, dx_last[None]])
    db = np.concatenate([db_, [db_last]])
    lams = np.zeros((k, xs.shape[1]), dtype=xs.dtype)
    munu = np.zeros((k, 2), dtype=xs.dtype)
    xi = -dxs[-1]
    lam_plus = np.zeros_like(xi)
    for j in range(k - 1, -1, -1):
        xplus, x = xs[j + 1], xs[j]
        xi = xi / b[j]
        mu = db[j] - lam_plus @ x + xplus @ xi
        nu = da[j] + x @ xi
        lam = -xi + mu * xplus + nu * x
        lams[j], munu[j] = lam, (mu, nu)
        xi = -dxs[j] - op.apply(lam, *params) + a[j] * lam + b[j] * lam_plus - b[j] * nu * xplus
        lam_plus = lam
    dvec = ((xi @ xs[0]) * xs[0] - xi) / np.linalg.norm(v)
    dparams = op.param_vjp(lams[::-1], xs[:k][::-1], *params)  # the oracle's order of summation: j = k - 1 first
    return dvec, dparams, lams, munu


def _over_probes(fn, probes):
    """[fn(b) for b in probes] on a few threads: numpy's longdouble loops release the interpreter lock"""
    if len(probes) == 1:
        return [fn(probes[0])]
    with ThreadPoolExecutor(max_workers=min(8, len(probes))) as pool:
        return list(pool.map(fn, probes))


def forward_pass(name, dtype, probes=None):
    """orc.tridiag_none in dtype for `probes` (default: all): xs (P, k + 1, n), alpha (P, k), beta (P, k)"""
    s = case_inputs(name)
    probes = list(range(s.p)) if probes is None else list(probes)
    op, params = oracle_operator(s, dtype)
    V = s.V.astype(dtype)

    def one(b):
        (xs, (a, b_)), (x_last, b_last) = orc.tridiag_none(op, s.k, V[b], *params)
        return np.concatenate([xs, x_last[None]]), a, np.concatenate([b_, [b_last]])

    got = _over_probes(one, probes)
    return tuple(np.stack([g[i] for g in got]) for i in range(3))


def adjoint_pass(name, dtype, probes, forward=None, dxs=None, dalpha=None, dbeta=None):
    """tridiag_none_vjp_states in dtype for `probes`, on the oracle's own forward pass or on forward = (xs, alpha, beta) holding
    one entry per entry of `probes`; cotangents default to those of case_inputs (arrays over ALL probes).
    Returns a dict: xs, alpha, beta, Lam (P, k, n), munu (P, k, 2), dv (P, n), grad (summed over `probes`)."""
    s = case_inputs(name)
    probes = list(probes)
    op, params = oracle_operator(s, dtype)
    V = s.V.astype(dtype)
    dxs, dalpha, dbeta = (np.asarray(s_ if given is None else given).astype(dtype)
                          for s_, given in ((s.dxs, dxs), (s.dalpha, dalpha), (s.dbeta, dbeta)))
    if forward is None:
        forward = forward_pass(name, dtype, probes)
    fwd = tuple(np.asarray(f).astype(dtype) for f in forward)

    def one(i):
        b = probes[i]
        return tridiag_none_vjp_states(op, s.k, V[b], params, cotangent(dxs[b], dalpha[b], dbeta[b]),
                                       forward=(fwd[0][i], fwd[1][i], fwd[2][i]))

    got = _over_probes(one, list(range(len(probes))))
    grad = got[0][1][0]
    for g in got[1:]:
        grad = grad + g[1][0]
    return {"xs": fwd[0], "alpha": fwd[1], "beta": fwd[2], "Lam": np.stack([g[2] for g in got]), "munu": np.stack([g[3] for g in got]),
            "dv": np.stack([g[0] for g in got]), "grad": grad}


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name="longdouble"):
    """The oracle's forward and adjoint for reference_probes(name) in the numpy type named, computed once and shared: treat the
    arrays as read-only.  longdouble only for the dense cases (n <= DENSE_MAX_N)."""
    assert dtype_name != "longdouble" or case(name)[1] <= DENSE_MAX_N, name
    out = adjoint_pass(name, np.dtype(dtype_name).type, reference_probes(name))
    for a in out.values():
        a.setflags(write=False)
    return out


def rel_err(x, ref, per_probe=True):
    """max over the probes of max|x_b - ref_b| / max|ref_b| (per_probe: axis 0 is the probe), in longdouble"""
    x, ref = np.asarray(x, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    if not per_probe:
        x, ref = x[None], ref[None]
    axes = tuple(range(1, ref.ndim))
    return float((np.abs(x - ref).max(axis=axes) / np.abs(ref).max(axis=axes)).max())


def errors_between(a, b):
    """{output: rel_err} of two results of reference / adjoint_pass; b is the yardstick"""
    return {o: rel_err(a[o], b[o], per_probe=o != "grad") for o in OUTPUTS}


def measure(name):
    """{"float64": {output: e64}, "float32": {output: e32}} of a dense case: the oracle in that type against longdouble"""
    ld = reference(name, "longdouble")
    return {dt: errors_between(reference(name, dt), ld) for dt in ("float64", "float32")}


# ------------------------------------------------------------------------------------------------
# The bounds: 32 x the measured e64 / e32 (two significant digits), relative to the output's largest magnitude per probe.
# ------------------------------------------------------------------------------------------------
FACTOR = 32.0
FP64_CAP, FP32_CAP = 1e-10, 1e-3

DENSE_BOUNDS = {
    "one-wave-scalar": {
        "float64": {"xs": 7.3e-13, "alpha": 7.9e-14, "beta": 1.9e-14, "Lam": 4.3e-13, "dv": 4.5e-13, "grad": 4.2e-13},
        # e64:  xs 2.28e-14, alpha 2.46e-15, beta 6.08e-16, Lam 1.35e-14, dv 1.42e-14, grad 1.31e-14
        "float32": {"xs": 0.0002, "alpha": 2.2e-05, "beta": 5.5e-06, "Lam": 0.00016, "dv": 0.00012, "grad": 0.00015},
        # e32:  xs 6.15e-06, alpha 6.98e-07, beta 1.70e-07, Lam 4.94e-06, dv 3.84e-06, grad 4.73e-06
    },
    "one-wave-vector": {
        "float64": {"xs": 5.7e-13, "alpha": 5.3e-14, "beta": 1.6e-14, "Lam": 3.6e-13, "dv": 3.7e-13, "grad": 3e-13},
        # e64:  xs 1.78e-14, alpha 1.66e-15, beta 4.95e-16, Lam 1.13e-14, dv 1.15e-14, grad 9.49e-15
        "float32": {"xs": 0.00015, "alpha": 1.5e-05, "beta": 7.2e-06, "Lam": 0.00014, "dv": 0.00015, "grad": 0.00014},
        # e32:  xs 4.59e-06, alpha 4.60e-07, beta 2.26e-07, Lam 4.32e-06, dv 4.83e-06, grad 4.47e-06
    },
    "wg256-scalar": {
        "float64": {"xs": 3.9e-13, "alpha": 7.7e-14, "beta": 1.6e-14, "Lam": 3.4e-13, "dv": 3e-13, "grad": 1.7e-13},
        # e64:  xs 1.21e-14, alpha 2.39e-15, beta 4.93e-16, Lam 1.06e-14, dv 9.34e-15, grad 5.42e-15
        "float32": {"xs": 0.00013, "alpha": 1.5e-05, "beta": 8.5e-06, "Lam": 0.00011, "dv": 0.00012, "grad": 6.9e-05},
        # e32:  xs 4.12e-06, alpha 4.79e-07, beta 2.66e-07, Lam 3.44e-06, dv 3.61e-06, grad 2.15e-06
    },
    "wg256-vector": {
        "float64": {"xs": 4.3e-13, "alpha": 5.2e-14, "beta": 1.7e-14, "Lam": 3.7e-13, "dv": 3.5e-13, "grad": 1.5e-13},
        # e64:  xs 1.35e-14, alpha 1.61e-15, beta 5.39e-16, Lam 1.16e-14, dv 1.09e-14, grad 4.82e-15
        "float32": {"xs": 0.00017, "alpha": 1.6e-05, "beta": 5.3e-06, "Lam": 0.00011, "dv": 0.00011, "grad": 7.2e-05},
        # e32:  xs 5.45e-06, alpha 5.08e-07, beta 1.65e-07, Lam 3.55e-06, dv 3.51e-06, grad 2.24e-06
    },
    "wg256-coarse": {
        "float64": {"xs": 3.4e-13, "alpha": 1.2e-14, "beta": 1.2e-14, "Lam": 2.4e-13, "dv": 2.1e-13, "grad": 2.1e-13},
        # e64:  xs 1.05e-14, alpha 3.68e-16, beta 3.88e-16, Lam 7.54e-15, dv 6.70e-15, grad 6.64e-15
        "float32": {"xs": 0.0001, "alpha": 1e-05, "beta": 5.4e-06, "Lam": 9.1e-05, "dv": 0.00013, "grad": 7.3e-05},
        # e32:  xs 3.20e-06, alpha 3.14e-07, beta 1.69e-07, Lam 2.84e-06, dv 4.10e-06, grad 2.30e-06
    },
    "two-slices-scalar": {
        "float64": {"xs": 5.8e-13, "alpha": 6e-14, "beta": 1.4e-14, "Lam": 4.3e-13, "dv": 4.6e-13, "grad": 2.1e-13},
        # e64:  xs 1.81e-14, alpha 1.87e-15, beta 4.36e-16, Lam 1.33e-14, dv 1.44e-14, grad 6.54e-15
        "float32": {"xs": 0.00025, "alpha": 3.1e-05, "beta": 6.1e-06, "Lam": 0.00021, "dv": 0.00018, "grad": 0.00011},
        # e32:  xs 7.94e-06, alpha 9.62e-07, beta 1.92e-07, Lam 6.50e-06, dv 5.50e-06, grad 3.29e-06
    },
    "two-slices-vector": {
        "float64": {"xs": 6.6e-13, "alpha": 3.7e-14, "beta": 1.3e-14, "Lam": 4.7e-13, "dv": 5.1e-13, "grad": 2.2e-13},
        # e64:  xs 2.06e-14, alpha 1.17e-15, beta 4.03e-16, Lam 1.46e-14, dv 1.59e-14, grad 6.75e-15
        "float32": {"xs": 0.00025, "alpha": 2.2e-05, "beta": 6.2e-06, "Lam": 0.00022, "dv": 0.00031, "grad": 0.00011},
        # e32:  xs 7.75e-06, alpha 6.92e-07, beta 1.95e-07, Lam 6.94e-06, dv 9.60e-06, grad 3.38e-06
    },
    "depth-one": {
        "float64": {"xs": 2.2e-13, "alpha": 1.4e-14, "beta": 5.9e-15, "Lam": 1.5e-14, "dv": 2e-13, "grad": 1.3e-14},
        # e64:  xs 6.93e-15, alpha 4.50e-16, beta 1.83e-16, Lam 4.62e-16, dv 6.10e-15, grad 4.01e-16
        "float32": {"xs": 9.9e-05, "alpha": 2.9e-06, "beta": 1.3e-06, "Lam": 4.9e-06, "dv": 8.3e-05, "grad": 4.1e-06},
        # e32:  xs 3.10e-06, alpha 8.92e-08, beta 4.04e-08, Lam 1.53e-07, dv 2.59e-06, grad 1.29e-07
    },
}


def bounds(name, dtype_name):
    """{output: bound} of a case.  A sparse case is too large for a longdouble run: it takes, per output, the largest bound of the
    dense cases of its depth k -- or, where no dense case has that depth ("second-trip", k = 2), of the nearest greater depth:
    every further step adds rounding errors and removes none, so a bound measured at depth 4 is not below what depth 2 would give
    at the same size.  tests/test_lanczos_cases_host.py checks the inherited bounds against the case's own fp64 - fp32 difference."""
    if name in DENSE_BOUNDS:
        return DENSE_BOUNDS[name][dtype_name]
    k = case(name)[3]
    depth = min(c[3] for c in CASES if c[4] == "dense" and c[3] >= k)
    donors = [DENSE_BOUNDS[c[0]][dtype_name] for c in CASES if c[4] == "dense" and c[3] == depth]
    return {o: max(b[o] for b in donors) for o in OUTPUTS}


if __name__ == "__main__":  # the table, ready to paste
    print("DENSE_BOUNDS = {")
    for nm in DENSE_NAMES:
        e = measure(nm)
        print(f'    "{nm}": {{')
        for dt in ("float64", "float32"):
            row = ", ".join(f'"{o}": {float(f"{FACTOR * e[dt][o]:.1e}")!r}' for o in OUTPUTS)
            print(f'        "{dt}": {{{row}}},')
            print("        # e" + dt[-2:] + ":  " + ", ".join(f"{o} {e[dt][o]:.2e}" for o in OUTPUTS))
        print("    },")
    print("}")
