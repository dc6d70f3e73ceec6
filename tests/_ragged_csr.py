"""Ragged sparse test matrices, their fp64 references and error bounds, and the launch geometry of the fused CSR step -- plain
numpy, no GPU.  tests/test_ragged_csr_host.py checks this file against itself on the CPU; tests/test_gpu_operator_kernels.py
compares the HIP kernels with it.

The matrices exist to reach what a 5-point stencil never does: empty rows and columns, whole slices of empty rows, rows of
1 .. 64 entries around the 8-entry rounds of k_csr_apply and the 2/4/8-entry rounds of k_csr_step, and a transposed structure that
differs from the forward one."""

import numpy as np

DEFAULT_LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64)

# 0, 1, -1, 2, -2, ..., 31, -31, 32: the first L offsets are L consecutive integers, so they are distinct modulo every n >= L --
# a row capped at n entries never repeats a column, whatever n is.  Offset 0 comes first: every non-empty row stores its diagonal.
OFFSETS = tuple([0] + [s * d for d in range(1, 32) for s in (1, -1)] + [32])
assert len(OFFSETS) == 64 and len(set(OFFSETS)) == 64 and OFFSETS[0] == 0


def empty_rows(n, empty_runs=()):
    """mask of the rows ragged_csr leaves empty by construction: 0 and n - 1 (n > 2) and every (start, count) run"""
    mask = np.zeros(n, dtype=bool)
    if n > 2:
        mask[[0, n - 1]] = True
    for start, count in empty_runs:
        assert 0 <= start and start + count <= n, (start, count, n)
        mask[start : start + count] = True
    return mask


def full_column(n, empty_runs=()):
    """The column ragged_csr fills with 64 entries, or None when no 64 consecutive-offset rows are free of forced-empty rows.
    Column c is stored by the rows c - OFFSETS[j]: c - 32 .. c + 31 (no wrap-around is used)."""
    mask = empty_rows(n, empty_runs)
    for c in range(32, n - 31):
        if not mask[c - 32 : c + 32].any():
            return c
    return None


def ragged_csr(n, rng, lengths=DEFAULT_LENGTHS, empty_runs=()):
    """COO (row, col, vals) of a non-symmetric n x n matrix, entries sorted by row.

    Row i gets a length from `lengths` (cycled over the rows, then shuffled by rng, capped at n); its columns are
    (i + OFFSETS[j]) % n for j < length.  One column, full_column(n, empty_runs), is then made 64 entries long by raising the
    length of row c - OFFSETS[j] to at least j + 1 (a column of A is a row of A^T: the transposed structure gets its longest row
    too).  Rows 0 and n - 1 (n > 2) and the rows of every (start, count) in empty_runs are empty.  No row and no column has more
    than 64 entries: a column c only receives entries from the 64 rows c - OFFSETS[j].  Values: 0.3 * standard normal, + 3 on the
    diagonal."""
    lens = np.resize(np.asarray(lengths, dtype=np.int64), n)
    rng.shuffle(lens)
    lens = np.minimum(lens, n)
    c = full_column(n, empty_runs)
    if c is not None:
        for j, off in enumerate(OFFSETS):
            lens[c - off] = max(lens[c - off], j + 1)
    lens[empty_rows(n, empty_runs)] = 0
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    j = np.concatenate([np.arange(m) for m in lens]) if n else np.zeros(0, dtype=np.int64)
    col = (row + np.asarray(OFFSETS, dtype=np.int64)[j.astype(np.int64)]) % n
    vals = 0.3 * rng.standard_normal(len(row)) + np.where(row == col, 3.0, 0.0)
    return row, col, vals


def add_entries(row, col, vals, i, cols, rng):
    """the COO triple with row i given the further columns `cols` (none of them stored yet), values 0.3 * standard normal"""
    cols = np.asarray(cols, dtype=np.int64)
    assert not np.isin(cols, col[row == i]).any() and len(set(cols.tolist())) == len(cols)
    return (np.concatenate([row, np.full(len(cols), i, dtype=np.int64)]), np.concatenate([col, cols]),
            np.concatenate([vals, 0.3 * rng.standard_normal(len(cols))]))


def dense_of(row, col, vals, n):
    A = np.zeros((n, n), dtype=np.float64)
    np.add.at(A, (row, col), np.asarray(vals, dtype=np.float64))
    return A


def row_and_col_lengths(row, col, n):
    return np.bincount(row, minlength=n), np.bincount(col, minlength=n)


# ------------------------------------------------------------------------------------------------
# fp64 references on the dense matrix.  Vectors are rows: X (p, n).
# ------------------------------------------------------------------------------------------------
def apply_ref(A, X, transpose=False):
    """(ref, mag): rows of A X^T (or A^T X^T) and of |A| |X|^T, fp64"""
    M = A.T if transpose else A
    return X @ M.T, np.abs(X) @ np.abs(M).T


def outer_ref(L, R):
    """(ref, mag): L^T R and |L|^T |R| for L, R (batch, n), fp64 -- the parameter-gradient sweep before sampling on a pattern"""
    return L.T @ R, np.abs(L).T @ np.abs(R)


def unit_roundoff(dtype_name):
    return {"float32": 2.0**-24, "float64": 2.0**-53}[dtype_name]


def apply_bound(m, u, mag):
    """Componentwise bound on |y_i - ref_i| for y_i = sum of m_i products a_ij x_j computed in a format of unit roundoff u, in ANY
    order of summation: 2 (m_i + 8) u (|A| |x|)_i.

    Derivation.  Each product carries one rounding, (1 + d), |d| <= u.  Whatever the order, a term passes through at most m_i - 1
    additions (a chain; a tree has fewer), each (1 + d): the computed sum is sum_j a_ij x_j (1 + theta_j) with
    |theta_j| <= gamma_{m_i} = m_i u / (1 - m_i u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.3 and
    the remark that it holds for every ordering).  The kernels end in a reduction tree over lanes, waves or LDS partials of at most
    8 further additions per term (64 lanes: 6, four waves: 2; 8 lanes: 3), hence m_i + 8.  For m_i u < 1/2 -- m_i <= 2^22 in fp32 --
    gamma_{m_i + 8} <= 2 (m_i + 8) u, which also absorbs the rounding of the fp64 reference itself (u64 << u) and, for fp32, of the
    operands, which are rounded to fp32 BEFORE the reference is formed.  A fused multiply-add only removes roundings.
    An output with no terms has mag = 0: the bound is 0 and the kernel must return exactly 0."""
    return 2.0 * (np.asarray(m, dtype=np.float64) + 8.0) * u * mag


def grad_bound(batch, u, mag, prefill):
    """Componentwise bound on |g_e - (prefill_e + ref_e)| for g_e = prefill_e + T(sum_b L_be R_be') with the sum in fp64:
    (2 batch u64 + 2 u) (|L|^T |R|)_e + u |prefill_e|.

    Derivation.  The fp64 products of operands of type T are exact for fp32 (24 + 24 bits) and carry one u64 rounding for fp64; the
    `batch`-term fp64 chain adds gamma_batch(u64) <= 2 batch u64 relative to |L|^T |R| (as apply_bound).  Rounding the sum s to T:
    |fl(s) - s| <= u |s| <= u (|L|^T |R|)_e.  The final add in T: |fl(a + fl(s)) - (a + fl(s))| <= u |a + fl(s)| <=
    u |prefill_e| + u (1 + u) (|L|^T |R|)_e.  Summed: (2 batch u64 + u + u (1 + u)) mag + u |prefill| <= the bound.  For T = fp64
    the cast is exact and the bound is merely loose."""
    return (2.0 * batch * unit_roundoff("float64") + 2.0 * u) * mag + u * np.abs(prefill)


# ------------------------------------------------------------------------------------------------
# launch geometry of the vector kernels and the fused CSR step (csrc/mfx_vec.h: pick_wg, Ctx, Ctx::fine, MFX_VEC_EPT_SWITCH)
# ------------------------------------------------------------------------------------------------
K_SLICE, K_EPT, K_BLOCK = 2048, 8, 256
VEC_WIDTH = {"float32": 4, "float64": 2}


def csr_step_geometry(n, p, dtype_name, aligned=True):
    """(wg, VEC, EPT) of k_csr_step for p vectors of length n: a workgroup owns wg * EPT consecutive rows (its slice).
    aligned: every vector the driver passes starts on a 16-byte boundary (true for whole torch allocations)."""
    wg = K_BLOCK if -(-n // K_SLICE) * p >= 16 else 64  # pick_wg
    width = VEC_WIDTH[dtype_name]
    vec = width if (n % width == 0 and aligned) else 1  # pick_vec
    nblk = -(-n // (wg * K_EPT))  # Ctx
    ept = K_EPT
    if vec > 1 and wg == K_BLOCK and nblk * p < 128:  # Ctx::fine
        ept = width
    if vec > 1 and ept != K_EPT:  # MFX_VEC_EPT_SWITCH
        return wg, width, width
    return (wg, width, K_EPT) if vec > 1 else (wg, 1, K_EPT)


def geometry_name(n, p, dtype_name):
    wg, vec, ept = csr_step_geometry(n, p, dtype_name)
    return f"wg{wg}-vec{vec}-ept{ept}"


def all_geometries(dtype_name):
    w = VEC_WIDTH[dtype_name]
    return {(64, 1, K_EPT), (64, w, K_EPT), (K_BLOCK, 1, K_EPT), (K_BLOCK, w, w), (K_BLOCK, w, K_EPT)}


# ------------------------------------------------------------------------------------------------
# The Krylov cases of tests/test_gpu_operator_kernels.py.  (n, p) come from the rules above; the empty run covers the rows of
# one whole workgroup of that geometry (longest == 0 in every thread of it) wherever n leaves at least one more slice with
# entries, and as much of the only slice as still leaves a matrix otherwise.
#   slice = wg * EPT rows: 512 (one wave), 2048 (256 threads, EPT 8), 1024 / 512 (256 threads, fine, fp32 / fp64)
# `seed` feeds the generator; the host test asserts the no-breakdown margins for every case, depth and probe.
# ------------------------------------------------------------------------------------------------
KRYLOV_DEPTHS = (1, 4, 9)

KRYLOV_CASES = (
    # name                n     p    empty run     seed
    ("one-wave-scalar", 1531, 1, (512, 512), 11),    # slices of 512: slice 1 is empty, slice 2 is ragged (507 rows)
    ("one-wave-vector", 1536, 1, (1024, 512), 12),   # the last slice is empty
    ("wg256-scalar", 1027, 16, (200, 600), 13),      # one slice of 2048 holds the whole matrix: 600 of its rows empty
    ("wg256-fine", 1028, 16, (0, 512), 14),          # fp64: slice 0 (512 rows) empty; fp32: half of slice 0 (1024 rows)
    ("wg256-coarse", 1028, 128, (300, 600), 15),     # EPT 8 with 16-byte loads; one slice of 2048
    ("wg256-scalar-two-slices", 3075, 16, (2048, 1027), 16),  # the ragged second slice of 2048 is empty
    ("wg256-fine-two-slices", 3076, 16, (1024, 1024), 17),    # fp32: slice 1 of 1024 empty; fp64: slices 2 and 3 of 512
    ("wg256-coarse-two-slices", 2052, 64, (2048, 4), 18),     # 2 slices x 64 vectors = 128 workgroups: coarse; the 4-row tail slice empty
)
TABLE_CASES = KRYLOV_CASES[:5]  # the five geometries, one case each


def krylov_case(name):
    """(row, col, vals, V) of a Krylov case: the matrix and its p start vectors, deterministic"""
    _, n, p, run, seed = next(c for c in KRYLOV_CASES if c[0] == name)
    rng = np.random.default_rng(seed)
    row, col, vals = ragged_csr(n, rng, empty_runs=(run,))
    return row, col, vals, rng.standard_normal((p, n))


def oracle_probes(p):
    """the probes compared with the CPU oracle one by one: all of them up to 16, else the first, two in the middle and the last"""
    return list(range(p)) if p <= 16 else [0, p // 3, (2 * p) // 3, p - 1]


def krylov_switch_case(longest):
    """The n = 1536 matrix of the "one-wave-vector" case with its longest row at 64 (as generated), 65 or 200 entries.
    65: a 64-entry row away from the full column gets that column too -- one row AND one column of 65, max_row_nnz == 65, the
    8-lanes-per-row path.  200: one row is filled up to 200 entries in columns that stay at most 64 long; the mean row length stays
    under 24, so with max_row_nnz unstated (0) the mean rule keeps the fused step and one thread walks the 200 entries."""
    n = 1536
    row, col, vals, _ = krylov_case("one-wave-vector")
    if longest == 64:
        return row, col, vals
    rows, cols = row_and_col_lengths(row, col, n)
    c = full_column(n, ((1024, 512),))
    i = next(int(i) for i in np.flatnonzero(rows == 64) if abs(int(i) - c) > 32)
    rng = np.random.default_rng(65)
    if longest == 65:
        extra = [c]
    else:
        free = np.setdiff1d(np.flatnonzero(cols < 64), col[row == i])
        extra = free[np.linspace(0, len(free) - 1, longest - 64).astype(np.int64)]
    row, col, vals = add_entries(row, col, vals, i, extra, rng)
    order = np.argsort(row * n + col, kind="stable")
    return row[order], col[order], vals[order]


def krylov_switch_vector():
    return np.random.default_rng(66).standard_normal(1536)
