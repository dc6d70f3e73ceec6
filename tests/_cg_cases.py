"""Cases, references, launch geometry and error bounds for csrc/mfx_cg.hip: mfx_pcg_solve (fixed-step and adaptive),
mfx_pcg_solve_reortho, mfx_precond_apply and mfx_partial_cholesky -- plain numpy, no GPU.
tests/test_cg_cases_host.py checks this file against itself and the oracle on the CPU; tests/test_gpu_cg_kernels.py compares
the HIP kernels with it.

Every input (matrix, right-hand sides, the factor Lt, minv, the Gram inputs and hyper-parameters, atol, rtol) is rounded to
float32 once, so it is exactly representable in float32, float64 and longdouble alike: one longdouble reference serves the
kernels of both types.

The oracle (oracle/slq_oracle.py) runs in longdouble as it stands for orc.pcg_fixed_step, orc.pcg_fixed_step_reortho and
orc._pcg_body.  Three things are restated here, and pinned to the oracle in float64 by the host test:
  * pcg_adaptive_trace: the loop of orc.pcg_adaptive around orc._pcg_body, keeping the stopping measure of every step;
  * cholesky_partial: orc.cholesky_partial and orc.cholesky_partial_pivot allocate float64 and ask for one element per call;
    this one keeps the float type, takes whole columns, and works in the original row order like the kernels;
  * woodbury_apply: orc.precondition_solve goes through scipy's float64 Cholesky.  The kernels receive minv, so the reference
    is the same expression z = (v - L minv L^T v) / s on the SAME rounded minv; with the unrounded minv it is
    orc.precondition_solve (host test).

BOUNDS does not come from the kernels.  Every entry is 32 times the error of the numpy oracle run in the same floating-point
type against the oracle run in longdouble, relative to the largest magnitude of the reference output per vector, measured on
the CPU: `python tests/_cg_cases.py` prints the table, the host test re-measures it and asserts that every stored bound lies
within [16, 64] times the measurement.  The factor 32 covers the different order of summation (kernels: per thread, wave,
slice; numpy: pairwise or BLAS blocks): the two errors are of one size, not equal."""

import functools
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _lanczos_cases as lc
import _ragged_csr as rc
from oracle import slq_oracle as orc

FACTOR = 32.0
FP64_CAP, FP32_CAP = 1e-10, 1e-3
DTYPES = ("float64", "float32")
SHIFT = 1.0  # s of the preconditioner s I + L L^T, every case
_f32 = lc._f32
rel_err = lc.rel_err


def _over(fn, items):
    items = list(items)
    if len(items) == 1:
        return [fn(items[0])]
    with ThreadPoolExecutor(max_workers=min(8, len(items))) as pool:
        return list(pool.map(fn, items))


# ------------------------------------------------------------------------------------------------
# launch geometry (csrc/mfx_vec.h: pick_wg, pick_vec, Ctx -- restated once, in tests/_ragged_csr.py)
# ------------------------------------------------------------------------------------------------
def cg_geometry(n, p, dtype_name, aligned=True):
    """(wg, VEC, nblk) of the vector kernels of pcg_t and precond_apply_t.  They go through MFX_VEC_SWITCH and never call
    Ctx::fine(): EPT is always kEpt, a slice holds wg * kEpt elements, nblk slices give nblk partial sums per dot."""
    wg, vec, _ = rc.csr_step_geometry(n, p, dtype_name, aligned)
    return wg, vec, -(-n // (wg * rc.K_EPT))


def claim_holds(token, n, p, rank, dtype_name):
    """whether the restated geometry of (n, p, rank) in this type has the property a case line names"""
    wg, vec, nblk = cg_geometry(n, p, dtype_name)
    return {
        "wg64": wg == 64,
        "wg256": wg == 256,
        "scalar": vec == 1,                                   # n is no multiple of the 16-byte width
        "vector": vec == rc.VEC_WIDTH[dtype_name],
        "ragged": n % (wg * rc.K_EPT) != 0,                   # the last slice is partly out of range
        "one-slice": nblk == 1,
        "two-slices": nblk == 2,
        "three-slices": nblk == 3,
        "more-slices-than-lanes": 64 < nblk <= 512,           # reduce_partials_group<T, 64>: second load slot, one trip
        "second-trip": nblk > 512,                            # its loop runs twice
        "jt-remainder-only": 1 <= rank < 4,                   # k_pre_finish: JT = 4
        "jt-full": rank >= 4 and rank % 4 == 0,
        "jt-full-and-remainder": rank > 4 and rank % 4 != 0,
        "second-stride": 256 < rank <= 512,                   # k_pre_small: for (i = tid; i < rank; i += 256)
        "rank-limit": rank == 1024,                           # check_precond
    }[token]


SOLVE_CASES = (
    # name                  n        p   rank steps operator   the branches the case is there for
    ("one-wave-scalar", 1531, 1, 3, 8, "dense", ("wg64", "scalar", "three-slices", "ragged", "jt-remainder-only")),
    ("one-wave-vector", 1536, 1, 4, 8, "dense", ("wg64", "vector", "three-slices", "jt-full")),
    ("wg256-scalar", 1027, 16, 257, 4, "dense", ("wg256", "scalar", "one-slice", "ragged", "second-stride")),
    ("wg256-vector", 1028, 16, 5, 4, "dense", ("wg256", "vector", "one-slice", "jt-full-and-remainder")),
    ("two-slices-scalar", 3075, 16, 1, 4, "dense", ("wg256", "scalar", "two-slices", "ragged", "jt-remainder-only")),
    ("two-slices-vector", 3076, 16, 5, 4, "dense", ("wg256", "vector", "two-slices", "ragged", "jt-full-and-remainder")),
    ("rank-limit", 1028, 1, 1024, 2, "dense", ("wg64", "vector", "three-slices", "rank-limit")),
    ("many-slices-scalar", 133121, 1, 5, 4, "sparse", ("wg256", "scalar", "more-slices-than-lanes", "ragged")),
    ("many-slices-vector", 133124, 1, 5, 4, "sparse", ("wg256", "vector", "more-slices-than-lanes", "ragged")),
    ("second-trip", 1050628, 1, 5, 2, "sparse", ("wg256", "vector", "second-trip", "ragged")),
)
SOLVE_NAMES = tuple(c[0] for c in SOLVE_CASES)
APPLY_NAMES = SOLVE_NAMES[:8]  # mfx_precond_apply: every rank above, one and four waves, and 66 slices
APPLY_P = 17


def solve_case(name):
    return next(c for c in SOLVE_CASES if c[0] == name)


def solve_id(name):
    _, n, p, rank, steps, _, _ = solve_case(name)
    parts = [f"{name}-n{n}-p{p}-rank{rank}-steps{steps}"]
    for dt, short in (("float32", "f32"), ("float64", "f64")):
        wg, vec, nblk = cg_geometry(n, p, dt)
        parts.append(f"{short}:wg{wg}.vec{vec}.nblk{nblk}")
    return "-".join(parts)


# ------------------------------------------------------------------------------------------------
# operators, preconditioners and inputs
# ------------------------------------------------------------------------------------------------
def dense_spd(n, seed, lo=1.0, hi=10.0):
    """orc.symmetric_matrix_from_eigenvalues with n eigenvalues spread evenly over [lo, hi], symmetrised and rounded to float32"""
    A = orc.symmetric_matrix_from_eigenvalues(np.linspace(lo, hi, n), seed=seed)
    return _f32(0.5 * (A + A.T))


def cholesky_partial(column, diagonal, n, rank, dtype, pivot):
    """orc.cholesky_partial (pivot False) / orc.cholesky_partial_pivot (True) in the float type `dtype`, from whole columns:
    column(k) -> K[:, k], diagonal() -> diag K, both in dtype.  Works in the original row order (the oracle permutes rows and
    undoes it at the end: the same numbers).  -> (L (n, rank), pivots, success, margins): margins[i] = (winner, runner-up) of
    the residual diagonal |d_j - sum_c L_jc^2| at step i (pivot only).  argmax takes the first index of a tie."""
    L = np.zeros((n, rank), dtype=dtype)
    diag = diagonal()
    pivots, margins, success = [], [], True
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(rank):
            k = i
            if pivot:
                res = np.abs(diag - np.einsum("jc,jc->j", L[:, :i], L[:, :i]))
                k = int(np.argmax(res))
                others = np.delete(res, k)
                margins.append((res[k], others.max() if len(others) else res[k] * 0))
            lrow = L[k, :i].copy()
            l2 = diag[k] - lrow @ lrow
            success = bool(success and l2 > 0.0)
            L[:, i] = (column(k) - L[:, :i] @ lrow) / np.sqrt(l2)
            pivots.append(k)
    return L, np.array(pivots, dtype=np.int64), success, margins


def dense_columns(A):
    return (lambda k: A[:, k]), (lambda: np.diagonal(A).copy())


def _matmul_rows(A, B):
    """A @ B in longdouble on a few threads (numpy's longdouble loops release the interpreter lock)"""
    blocks = np.array_split(np.arange(A.shape[0]), 8)
    return np.concatenate(_over(lambda rows: A[rows] @ B, [b for b in blocks if len(b)]))


def inverse_spd(C):
    """C^-1 of a symmetric positive definite longdouble matrix by its Cholesky factor, in longdouble"""
    C = np.array(C, dtype=np.longdouble)
    r = len(C)
    G = np.zeros_like(C)
    for j in range(r):
        col = C[j:, j] / np.sqrt(C[j, j])
        G[j:, j] = col
        C[j + 1:, j + 1:] -= np.outer(col[1:], col[1:])

    def solve(cols):  # G G^T X = I on a block of columns
        Y = np.zeros((r, len(cols)), dtype=np.longdouble)
        for i in range(r):
            Y[i] = ((cols == i) - G[i, :i] @ Y[:i]) / G[i, i]
        for i in range(r - 1, -1, -1):
            Y[i] = (Y[i] - G[i + 1:, i] @ Y[i + 1:]) / G[i, i]
        return Y

    blocks = [b for b in np.array_split(np.arange(r), 8) if len(b)]
    X = np.concatenate(_over(solve, blocks), axis=1)
    return 0.5 * (X + X.T)


def minv_of(Lt, shift=SHIFT):
    """(s I + L^T L)^-1 in longdouble, symmetric, rounded to float32; Lt (rank, n) holds float32 values"""
    Ld = Lt.astype(np.longdouble)
    return _f32(inverse_spd(_matmul_rows(Ld, Ld.T) + np.longdouble(shift) * np.eye(len(Lt), dtype=np.longdouble)))


def dense_factor(A, rank):
    """Lt (rank, n): the longdouble pivoted partial Cholesky factor of A, transposed, rounded to float32"""
    col, diag = dense_columns(A.astype(np.longdouble))
    L, _, success, _ = cholesky_partial(col, diag, len(A), rank, np.longdouble, True)
    assert success
    return np.ascontiguousarray(_f32(L.T))


@functools.lru_cache(maxsize=None)
def solve_inputs(name):
    """operator, right-hand sides B (p, n), the preconditioner (Lt, minv) and APPLY_P vectors V for mfx_precond_apply"""
    idx = SOLVE_NAMES.index(name)
    _, n, p, rank, steps, kind, _ = solve_case(name)
    rng = np.random.default_rng(5200 + idx)
    s = types.SimpleNamespace(name=name, n=n, p=p, rank=rank, steps=steps, kind=kind)
    if kind == "dense":
        s.A = dense_spd(n, seed=5300 + idx)
        s.Lt = dense_factor(s.A, rank)
    else:
        s.row, s.col, s.vals = lc.sparse_coo(n, rng)
        s.Lt = _f32(rng.standard_normal((rank, n)) / np.sqrt(n))  # a random factor: L L^T has eigenvalues of order 1
    s.minv = minv_of(s.Lt)
    s.B = _f32(rng.standard_normal((p, n)))
    if name in APPLY_NAMES:
        s.V = _f32(rng.standard_normal((APPLY_P, n)))
    return s


def matvec(s, dtype):
    if s.kind == "dense":
        A = s.A.astype(dtype)
        return lambda v: A @ v
    op, vals = orc.CooOp(s.row, s.col, s.n), s.vals.astype(dtype)
    return lambda v: op.apply(v, vals)


def woodbury_apply(Lt, minv, shift, v):
    """z = (v - L minv L^T v) / s in the float type of the arguments; minv symmetric"""
    return (v - (minv @ (Lt @ v)) @ Lt) / shift


def preconditioner(s, dtype):
    Lt, minv, shift = s.Lt.astype(dtype), s.minv.astype(dtype), dtype(SHIFT)
    return lambda v: woodbury_apply(Lt, minv, shift, v)


# ------------------------------------------------------------------------------------------------
# the adaptive batch and the re-orthogonalising cases: n = 1000, one wave, two slices of 512, 16-byte loads
# ------------------------------------------------------------------------------------------------
ADAPTIVE_N, ADAPTIVE_RANK, ADAPTIVE_MAXITER = 1000, 5, 8
ADAPTIVE_ATOL = ADAPTIVE_RTOL = 2.0**-7
ADAPTIVE_SCALES = (64.0, 0.03125, 0.2421875)  # columns that stop after 4, 1 and 2 steps; see adaptive_inputs
REORTHO_CASES = (
    # name          n    p  rank  num_matvecs
    ("rank-below", 1000, 2, 5, 8),   # kdim = num_matvecs: the basis rows outnumber the factor's
    ("rank-above", 1000, 2, 12, 8),  # kdim = rank
    ("plain", 1000, 2, 0, 8),        # no preconditioner: z is r
)
REORTHO_NAMES = tuple(c[0] for c in REORTHO_CASES)


@functools.lru_cache(maxsize=None)
def small_inputs(rank, seed, hi):
    """dense SPD matrix of ADAPTIVE_N rows with eigenvalues in [1, hi], its factor of the given rank (0: none) and minv.
    hi = 1.25 (adaptive): the stopping measure falls by more than 4 a step, so it can jump over [1/2, 2].  hi = 10
    (re-orthogonalising, 8 steps): the last residual stays far above the rounding level of float32."""
    s = types.SimpleNamespace(n=ADAPTIVE_N, rank=rank, kind="dense")
    s.A = dense_spd(s.n, seed=seed, lo=1.0, hi=hi)
    if rank:
        s.Lt = dense_factor(s.A, rank)
        s.minv = minv_of(s.Lt)
    return s


@functools.lru_cache(maxsize=None)
def adaptive_inputs():
    """Three right-hand sides of different length, hence different difficulty against atol: column 0, a long random vector,
    stops after 4 steps; column 1, a short one, after 1; column 2, within the span of three eigenvectors, after 2.  The lengths
    were chosen on the longdouble oracle so that no stopping measure of any step lies in [1/2, 2] (host test)."""
    s = small_inputs(ADAPTIVE_RANK, 5400, 1.25)
    rng = np.random.default_rng(5401)
    g = rng.standard_normal((3, s.n))
    w, U = np.linalg.eigh(s.A)
    g[2] = U[:, [10, 500, 990]] @ np.array([1.0, -2.0, 1.5]) * np.sqrt(s.n / 7.25)
    s.B = _f32(g * np.array(ADAPTIVE_SCALES)[:, None])
    s.p = 3
    return s


def pcg_adaptive_trace(A, b, P=None, *, atol, rtol, maxiter, miniter=0):
    """orc.pcg_adaptive, also returning r and the stopping measure rms(r / (atol + |x| rtol)) it evaluated before every step and
    at the end -> (x, r, num_steps, measures (num_steps + 1,))"""
    P = (lambda v: v) if P is None else P
    x = np.zeros_like(b)
    r = b - A(x)
    z = P(r)
    state, nsteps, measures = (x, z, r, z), 0, []
    while True:
        x, _p, r, _z = state
        error_rel = r / (atol + np.abs(x) * rtol)
        measures.append(np.sqrt(np.mean(error_rel**2)))
        if not ((measures[-1] > 1.0 or nsteps < miniter) and nsteps < maxiter):
            break
        state = orc._pcg_body(A, P, state)
        nsteps += 1
    return state[0], state[2], nsteps, np.array(measures)


@functools.lru_cache(maxsize=None)
def reortho_inputs(name):
    _, n, p, rank, m = next(c for c in REORTHO_CASES if c[0] == name)
    s = small_inputs(rank, 5500 + REORTHO_NAMES.index(name), 10.0)
    rng = np.random.default_rng(5510 + REORTHO_NAMES.index(name))
    return types.SimpleNamespace(**vars(s), p=p, m=m, B=_f32(rng.standard_normal((p, n))))


# ------------------------------------------------------------------------------------------------
# partial Cholesky
# ------------------------------------------------------------------------------------------------
GRAM_LS, GRAM_OS, GRAM_NOISE, GRAM_D = 0.75, 1.5, 0.25, 2
CHOL_CASES = (
    # name            n   rank operator pivot with_noise
    ("dense-255-pivot", 255, 4, "dense", 1, 0),     # one block of 256 rows, ragged
    ("dense-256-pivot", 256, 4, "dense", 1, 0),     # one full block
    ("dense-257-pivot", 257, 4, "dense", 1, 0),     # a second block of one row, which holds the first pivot
    ("dense-257-plain", 257, 4, "dense", 0, 0),
    ("gram-255-pivot", 255, 4, "gram", 1, 0),
    ("gram-256-pivot", 256, 4, "gram", 1, 1),
    ("gram-257-pivot", 257, 4, "gram", 1, 0),
    ("gram-257-plain", 257, 4, "gram", 0, 1),
    ("gram-65537-pivot", 65537, 4, "gram", 1, 0),   # nparts = 257 > 256: second trip of the cross-block loop of k_pchol_col,
    ("gram-65537-plain", 65537, 4, "gram", 0, 1),   # and its last block holds the first pivot
)
CHOL_NAMES = tuple(c[0] for c in CHOL_CASES)
TIE_PIVOTS = (7, 300, 555, 10)


def chol_case(name):
    return next(c for c in CHOL_CASES if c[0] == name)


def expected_pivots(name):
    """what the construction of chol_inputs aims at (the host test asserts the longdouble oracle finds exactly these)"""
    _, n, rank, kind, pivot, _ = chol_case(name)
    if not pivot:
        return tuple(range(rank))
    return (n - 1, n // 2, 100, 7) if kind == "dense" else (0, n - 1, n // 2, 100)


@functools.lru_cache(maxsize=None)
def chol_inputs(name):
    """dense: an SPD matrix with eigenvalues in [1, 10] whose diagonal is raised by 8, 6, 4.5 and 3.25 in four rows -- the pivots,
    one of them in the last block.  gram: RBF kernel on a cluster of points in [0, 0.25]^2 and three outliers at different
    distances from it, one of them the last point.  Every diagonal entry of a Gram matrix is the same number, so its step 0 is an
    exact tie of all n rows, in every type: row 0 wins it; from step 1 on the outliers win by a wide margin."""
    idx = CHOL_NAMES.index(name)
    _, n, rank, kind, pivot, with_noise = chol_case(name)
    rng = np.random.default_rng(5600 + idx)
    s = types.SimpleNamespace(name=name, n=n, rank=rank, kind=kind, pivot=pivot, with_noise=with_noise)
    if kind == "dense":
        A = orc.symmetric_matrix_from_eigenvalues(np.linspace(1.0, 10.0, n), seed=5700 + idx)
        A = 0.5 * (A + A.T)
        A[(n - 1, n // 2, 100, 7), (n - 1, n // 2, 100, 7)] += (8.0, 6.0, 4.5, 3.25)
        s.A = _f32(A)
    else:
        X = rng.uniform(0.0, 0.25, (n, GRAM_D))
        X[[n - 1, n // 2, 100]] = [[1.5, 0.0], [0.0, -1.125], [-0.75, 0.375]]
        s.X = _f32(X)
    return s


def chol_columns(s, dtype):
    """(column, diagonal) of cholesky_partial for a case, in dtype.  gram: one column of orc.kernel_matrix at a time, never the
    n x n matrix; the diagonal is outputscale (+ noise): the distance of a point to itself is exactly 0, as in the kernels."""
    if s.kind != "gram":
        return dense_columns(s.A.astype(dtype))
    X, ls, os_, noise = s.X.astype(dtype), dtype(GRAM_LS), dtype(GRAM_OS), dtype(GRAM_NOISE if s.with_noise else 0.0)

    def column(k):
        c = orc.kernel_matrix("rbf", X, X[k:k + 1], ls, os_)[:, 0].astype(dtype)
        c[k] = os_ + noise
        return c

    return column, (lambda: np.full(s.n, os_ + noise, dtype=dtype))


def tie_matrix():
    """600 x 600 small integers, block diagonal: 16 on the diagonal at rows 7, 300, 555 (three different blocks of 256 rows), 9 at
    rows 10 and 260, 2 at row 9, 1 elsewhere; A[7, 9] = 4, A[300, 301] = 3.  Every step of the pivoted factorisation is exact in
    float32 (square roots 4, 4, 4, 3); steps 0, 1 and 3 are ties, which the first index wins: pivots 7, 300, 555, 10."""
    A = np.eye(600)
    A[[7, 300, 555], [7, 300, 555]] = 16.0
    A[[10, 260], [10, 260]] = 9.0
    A[9, 9] = 2.0
    A[7, 9] = A[9, 7] = 4.0
    A[300, 301] = A[301, 300] = 3.0
    return A


def deficient_matrix():
    """300 x 300, v v^T for a vector of small integers with v_0 = 2 and the largest entry v_5 = 4: exactly rank one.  Without
    pivoting column 0 is v and step 1 meets the residual 0: success = 0.  With pivoting column 0 is v again (pivot 5)."""
    v = np.resize(np.array([2.0, 1.0, -1.0, 3.0, -2.0, 1.0, 2.0]), 300)
    v[5] = 4.0
    return np.outer(v, v), v


# ------------------------------------------------------------------------------------------------
# one table of everything that is measured: key -> outputs in a float type
# ------------------------------------------------------------------------------------------------
def keys():
    out = [f"solve/{nm}/{v}" for nm in SOLVE_NAMES for v in ("plain", "pre")]
    out += ["adaptive"] + [f"reortho/{nm}" for nm in REORTHO_NAMES]
    out += [f"apply/{nm}" for nm in APPLY_NAMES] + [f"chol/{nm}" for nm in CHOL_NAMES]
    return tuple(out)


def outputs_of(key):
    kind = key.split("/")[0]
    return {"solve": ("x", "r"), "adaptive": ("x",), "reortho": ("x", "r", "q"), "apply": ("z",), "chol": ("Lt",)}[kind]


@functools.lru_cache(maxsize=None)
def run(key, dtype_name="longdouble"):
    """The oracle's outputs for a key in the numpy type named, computed once and shared: treat the arrays as read-only.
    Vectors are rows: x, r (p, n); q (p, num_matvecs, n); z (APPLY_P, n); Lt (rank, n).  adaptive: also num_steps, measures;
    chol: also pivots, success, margins."""
    dtype = np.dtype(dtype_name).type
    kind, _, rest = key.partition("/")
    if kind == "solve":
        name, variant = rest.split("/")
        s = solve_inputs(name)
        A, B, P = matvec(s, dtype), s.B.astype(dtype), preconditioner(s, dtype) if variant == "pre" else None
        got = _over(lambda b: orc.pcg_fixed_step(A, B[b], P, num_matvecs=s.steps), range(s.p))
        out = {"x": np.stack([g[0] for g in got]), "r": np.stack([g[1]["residual_abs"] for g in got])}
    elif kind == "adaptive":
        s = adaptive_inputs()
        A, B, P = matvec(s, dtype), s.B.astype(dtype), preconditioner(s, dtype)
        got = [pcg_adaptive_trace(A, B[b], P, atol=ADAPTIVE_ATOL, rtol=ADAPTIVE_RTOL, maxiter=ADAPTIVE_MAXITER) for b in range(s.p)]
        out = {"x": np.stack([g[0] for g in got]), "r": np.stack([g[1] for g in got]),
               "num_steps": np.array([g[2] for g in got]), "measures": tuple(g[3] for g in got)}
    elif kind == "reortho":
        s = reortho_inputs(rest)
        A, B, P = matvec(s, dtype), s.B.astype(dtype), preconditioner(s, dtype) if s.rank else None
        got = [orc.pcg_fixed_step_reortho(A, B[b], P, num_matvecs=s.m) for b in range(s.p)]
        out = {"x": np.stack([g[0] for g in got]), "r": np.stack([g[1]["residual_abs"] for g in got]),
               "q": np.stack([g[1]["Q"].T for g in got])}
    elif kind == "apply":
        s = solve_inputs(rest)
        P, V = preconditioner(s, dtype), s.V.astype(dtype)
        out = {"z": np.stack([P(v) for v in V])}
    else:
        s = chol_inputs(rest)
        column, diagonal = chol_columns(s, dtype)
        L, pivots, success, margins = cholesky_partial(column, diagonal, s.n, s.rank, dtype, bool(s.pivot))
        out = {"Lt": np.ascontiguousarray(L.T), "pivots": pivots, "success": success, "margins": margins}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def measure(key):
    """{"float64": {output: e64}, "float32": {output: e32}}: the oracle in that type against the oracle in longdouble"""
    ld = run(key)
    return {dt: {o: rel_err(run(key, dt)[o], ld[o]) for o in outputs_of(key)} for dt in DTYPES}


BOUNDS = {
    "solve/one-wave-scalar/plain": {
        "float64": {"x": 3.8e-14, "r": 2.2e-13},  # e: x 1.19e-15, r 6.86e-15
        "float32": {"x": 1.9e-05, "r": 9.1e-05},  # e: x 5.79e-07, r 2.85e-06
    },
    "solve/one-wave-scalar/pre": {
        "float64": {"x": 5.2e-14, "r": 2.1e-13},  # e: x 1.64e-15, r 6.64e-15
        "float32": {"x": 2.1e-05, "r": 0.00017},  # e: x 6.54e-07, r 5.23e-06
    },
    "solve/one-wave-vector/plain": {
        "float64": {"x": 3.5e-14, "r": 3.1e-13},  # e: x 1.09e-15, r 9.73e-15
        "float32": {"x": 1.5e-05, "r": 9.4e-05},  # e: x 4.78e-07, r 2.95e-06
    },
    "solve/one-wave-vector/pre": {
        "float64": {"x": 4.9e-14, "r": 9.6e-14},  # e: x 1.53e-15, r 3.01e-15
        "float32": {"x": 2.3e-05, "r": 9.5e-05},  # e: x 7.19e-07, r 2.95e-06
    },
    "solve/wg256-scalar/plain": {
        "float64": {"x": 5.2e-14, "r": 2.1e-13},  # e: x 1.62e-15, r 6.60e-15
        "float32": {"x": 2.2e-05, "r": 8.1e-05},  # e: x 6.78e-07, r 2.54e-06
    },
    "solve/wg256-scalar/pre": {
        "float64": {"x": 1e-13, "r": 5.3e-13},  # e: x 3.23e-15, r 1.66e-14
        "float32": {"x": 2.4e-05, "r": 0.00017},  # e: x 7.53e-07, r 5.25e-06
    },
    "solve/wg256-vector/plain": {
        "float64": {"x": 6.9e-14, "r": 2.1e-13},  # e: x 2.16e-15, r 6.66e-15
        "float32": {"x": 2.2e-05, "r": 0.00012},  # e: x 7.01e-07, r 3.75e-06
    },
    "solve/wg256-vector/pre": {
        "float64": {"x": 6.8e-14, "r": 2e-13},  # e: x 2.12e-15, r 6.23e-15
        "float32": {"x": 1.9e-05, "r": 4.7e-05},  # e: x 5.81e-07, r 1.48e-06
    },
    "solve/two-slices-scalar/plain": {
        "float64": {"x": 5.8e-14, "r": 2.6e-13},  # e: x 1.83e-15, r 8.04e-15
        "float32": {"x": 3.4e-05, "r": 0.00018},  # e: x 1.07e-06, r 5.67e-06
    },
    "solve/two-slices-scalar/pre": {
        "float64": {"x": 6.4e-14, "r": 2.3e-13},  # e: x 2.01e-15, r 7.19e-15
        "float32": {"x": 3.4e-05, "r": 0.00014},  # e: x 1.05e-06, r 4.49e-06
    },
    "solve/two-slices-vector/plain": {
        "float64": {"x": 1e-13, "r": 3.1e-13},  # e: x 3.12e-15, r 9.62e-15
        "float32": {"x": 3.2e-05, "r": 0.00016},  # e: x 9.90e-07, r 4.96e-06
    },
    "solve/two-slices-vector/pre": {
        "float64": {"x": 7.7e-14, "r": 6.9e-13},  # e: x 2.40e-15, r 2.14e-14
        "float32": {"x": 3.4e-05, "r": 0.00019},  # e: x 1.08e-06, r 6.02e-06
    },
    "solve/rank-limit/plain": {
        "float64": {"x": 3e-14, "r": 1e-13},  # e: x 9.39e-16, r 3.11e-15
        "float32": {"x": 1.6e-05, "r": 4.3e-05},  # e: x 4.85e-07, r 1.34e-06
    },
    "solve/rank-limit/pre": {
        "float64": {"x": 1.4e-13, "r": 1.3e-12},  # e: x 4.49e-15, r 4.07e-14
        "float32": {"x": 4.9e-05, "r": 0.00038},  # e: x 1.52e-06, r 1.19e-05
    },
    "solve/many-slices-scalar/plain": {
        "float64": {"x": 1.3e-14, "r": 9.7e-14},  # e: x 4.16e-16, r 3.04e-15
        "float32": {"x": 5.1e-06, "r": 4.8e-05},  # e: x 1.60e-07, r 1.51e-06
    },
    "solve/many-slices-scalar/pre": {
        "float64": {"x": 8.7e-15, "r": 6.7e-14},  # e: x 2.72e-16, r 2.08e-15
        "float32": {"x": 4.9e-06, "r": 6.7e-05},  # e: x 1.54e-07, r 2.11e-06
    },
    "solve/many-slices-vector/plain": {
        "float64": {"x": 9e-15, "r": 1.1e-13},  # e: x 2.80e-16, r 3.29e-15
        "float32": {"x": 4.6e-06, "r": 4.7e-05},  # e: x 1.45e-07, r 1.46e-06
    },
    "solve/many-slices-vector/pre": {
        "float64": {"x": 9.9e-15, "r": 8.7e-14},  # e: x 3.10e-16, r 2.71e-15
        "float32": {"x": 4.9e-06, "r": 3.8e-05},  # e: x 1.52e-07, r 1.20e-06
    },
    "solve/second-trip/plain": {
        "float64": {"x": 1.6e-14, "r": 7.3e-13},  # e: x 5.11e-16, r 2.27e-14
        "float32": {"x": 1.3e-05, "r": 0.00055},  # e: x 4.15e-07, r 1.72e-05
    },
    "solve/second-trip/pre": {
        "float64": {"x": 9.1e-15, "r": 1.1e-13},  # e: x 2.83e-16, r 3.31e-15
        "float32": {"x": 1.4e-05, "r": 0.00061},  # e: x 4.35e-07, r 1.89e-05
    },
    "adaptive": {
        "float64": {"x": 4.1e-14},  # e: x 1.27e-15
        "float32": {"x": 1.5e-05},  # e: x 4.80e-07
    },
    "reortho/rank-below": {
        "float64": {"x": 4.6e-14, "r": 2.8e-13, "q": 2.1e-13},  # e: x 1.44e-15, r 8.88e-15, q 6.47e-15
        "float32": {"x": 2.1e-05, "r": 0.00015, "q": 9.8e-05},  # e: x 6.58e-07, r 4.54e-06, q 3.07e-06
    },
    "reortho/rank-above": {
        "float64": {"x": 5.8e-14, "r": 7.2e-14, "q": 1e-13},  # e: x 1.81e-15, r 2.26e-15, q 3.24e-15
        "float32": {"x": 1.8e-05, "r": 6.9e-05, "q": 5e-05},  # e: x 5.60e-07, r 2.15e-06, q 1.58e-06
    },
    "reortho/plain": {
        "float64": {"x": 4.2e-14, "r": 2.5e-13, "q": 1.7e-13},  # e: x 1.33e-15, r 7.74e-15, q 5.25e-15
        "float32": {"x": 2.2e-05, "r": 9.8e-05, "q": 6.5e-05},  # e: x 6.80e-07, r 3.05e-06, q 2.02e-06
    },
    "apply/one-wave-scalar": {
        "float64": {"z": 2.2e-14},  # e: z 6.75e-16
        "float32": {"z": 1.5e-05},  # e: z 4.71e-07
    },
    "apply/one-wave-vector": {
        "float64": {"z": 2.5e-14},  # e: z 7.82e-16
        "float32": {"z": 5.4e-06},  # e: z 1.70e-07
    },
    "apply/wg256-scalar": {
        "float64": {"z": 5e-14},  # e: z 1.56e-15
        "float32": {"z": 1.3e-05},  # e: z 4.05e-07
    },
    "apply/wg256-vector": {
        "float64": {"z": 1.5e-14},  # e: z 4.83e-16
        "float32": {"z": 8.4e-06},  # e: z 2.61e-07
    },
    "apply/two-slices-scalar": {
        "float64": {"z": 7.5e-15},  # e: z 2.34e-16
        "float32": {"z": 3.8e-06},  # e: z 1.18e-07
    },
    "apply/two-slices-vector": {
        "float64": {"z": 2.8e-14},  # e: z 8.85e-16
        "float32": {"z": 1.1e-05},  # e: z 3.47e-07
    },
    "apply/rank-limit": {
        "float64": {"z": 2e-13},  # e: z 6.37e-15
        "float32": {"z": 9.8e-05},  # e: z 3.06e-06
    },
    "apply/many-slices-scalar": {
        "float64": {"z": 3.1e-15},  # e: z 9.56e-17
        "float32": {"z": 1.8e-06},  # e: z 5.48e-08
    },
    "chol/dense-255-pivot": {
        "float64": {"Lt": 2.5e-15},  # e: Lt 7.93e-17
        "float32": {"Lt": 2.3e-06},  # e: Lt 7.22e-08
    },
    "chol/dense-256-pivot": {
        "float64": {"Lt": 3.4e-15},  # e: Lt 1.05e-16
        "float32": {"Lt": 2.1e-06},  # e: Lt 6.49e-08
    },
    "chol/dense-257-pivot": {
        "float64": {"Lt": 2.6e-15},  # e: Lt 8.01e-17
        "float32": {"Lt": 1.9e-06},  # e: Lt 6.09e-08
    },
    "chol/dense-257-plain": {
        "float64": {"Lt": 4.7e-15},  # e: Lt 1.46e-16
        "float32": {"Lt": 1.6e-06},  # e: Lt 5.15e-08
    },
    "chol/gram-255-pivot": {
        "float64": {"Lt": 9.6e-15},  # e: Lt 3.00e-16
        "float32": {"Lt": 7.2e-06},  # e: Lt 2.24e-07
    },
    "chol/gram-256-pivot": {
        "float64": {"Lt": 7.8e-15},  # e: Lt 2.45e-16
        "float32": {"Lt": 5.6e-06},  # e: Lt 1.74e-07
    },
    "chol/gram-257-pivot": {
        "float64": {"Lt": 1.2e-14},  # e: Lt 3.79e-16
        "float32": {"Lt": 7.6e-06},  # e: Lt 2.39e-07
    },
    "chol/gram-257-plain": {
        "float64": {"Lt": 4e-14},  # e: Lt 1.24e-15
        "float32": {"Lt": 2.8e-05},  # e: Lt 8.69e-07
    },
    "chol/gram-65537-pivot": {
        "float64": {"Lt": 1.5e-14},  # e: Lt 4.70e-16
        "float32": {"Lt": 1.1e-05},  # e: Lt 3.42e-07
    },
    "chol/gram-65537-plain": {
        "float64": {"Lt": 4.8e-14},  # e: Lt 1.51e-15
        "float32": {"Lt": 3.5e-05},  # e: Lt 1.08e-06
    },
}


def bounds(key, dtype_name):
    return BOUNDS[key][dtype_name]


if __name__ == "__main__":  # the table, ready to paste
    print("BOUNDS = {")
    for key in keys():
        e = measure(key)
        print(f'    "{key}": {{')
        for dt in DTYPES:
            row = ", ".join(f'"{o}": {float(f"{FACTOR * e[dt][o]:.1e}")!r}' for o in outputs_of(key))
            print(f'        "{dt}": {{{row}}},  # e: ' + ", ".join(f"{o} {e[dt][o]:.2e}" for o in outputs_of(key)))
        print("    },")
    print("}")
