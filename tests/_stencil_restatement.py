"""NumPy restatement of the reference's stencil vector fields (util/pde_util.py:74-157), written from its text: the yardstick of
tests/test_stencil_host.py and tests/test_gpu_stencil.py.

  pad          np.pad(u, 1) (boundary_dirichlet, :146-150) or np.pad(u, 1, mode="edge") (boundary_neumann, :153-157)
  conv         convolve2d(stencil, padded, "valid") as its nine shifted slices: out[r, c] = sum_ab stencil[a, b] padded[r + 2 - a, c + 2 - b]
  block forms  heat: coef conv(u) (:74-87);  heat2: (-coef conv(u), du) (:106-123);  wave: (du, coef conv(u)) (:126-143)

Everything acts on the last two axes, so a stack of states goes through at once; the dense matrix is built column by column from
the identity.  `transpose_apply` restates the gather rule of the transposed operator (include/mfx.h)
independently of the dense matrix, cell by cell.
"""

import functools

import numpy as np

FORMS = ("heat", "heat2", "wave")
BOUNDARIES = ("dirichlet", "neumann")


def pad(u, boundary):
    width = [(0, 0)] * (u.ndim - 2) + [(1, 1), (1, 1)]
    return np.pad(u, width, mode="edge") if boundary == "neumann" else np.pad(u, width, mode="constant", constant_values=0.0)


def conv(stencil, u, boundary):
    """convolve2d(stencil, pad(u), mode="valid") on the last two axes"""
    ny, nx = u.shape[-2:]
    up = pad(u, boundary)
    out = np.zeros_like(u, dtype=np.result_type(u, np.float64))
    for a in range(3):
        for b in range(3):
            out = out + stencil[a, b] * up[..., 2 - a : 2 - a + ny, 2 - b : 2 - b + nx]
    return out


def apply(form, stencil, boundary, coef, x):
    """x (..., ny, nx) for heat, (..., 2, ny, nx) otherwise; coef (ny, nx) or None"""
    c = 1.0 if coef is None else coef
    if form == "heat":
        return c * conv(stencil, x, boundary)
    u, du = x[..., 0, :, :], x[..., 1, :, :]
    fx = c * conv(stencil, u, boundary)
    return np.stack([-fx, du], axis=-3) if form == "heat2" else np.stack([du, fx], axis=-3)


def state_size(form, ny, nx):
    return ny * nx if form == "heat" else 2 * ny * nx


def dense_matrix(form, stencil, boundary, coef, ny, nx):
    """A with A[:, j] = apply(e_j) on flattened states"""
    n = state_size(form, ny, nx)
    eye = np.eye(n).reshape((n, ny, nx) if form == "heat" else (n, 2, ny, nx))
    return apply(form, stencil, boundary, coef, eye).reshape(n, n).T.copy()


def abs_matrix(form, stencil, boundary, coef, ny, nx):
    """The operator of the absolute weights and the absolute field: sum over the (at most nine) products of |w| |coef|.  Entry by
    entry >= |dense_matrix|, and equal to it wherever the weights that the padding rule folds onto one cell have one sign."""
    A = dense_matrix(form, np.abs(stencil), boundary, None if coef is None else np.abs(coef), ny, nx)
    return np.abs(A)


def conv_matrix(stencil, boundary, ny, nx):
    """S alone, (ny nx, ny nx)"""
    return dense_matrix("heat", stencil, boundary, None, ny, nx)


def correlation_weights(stencil):
    """w[dr + 1, dc + 1] multiplies u_pad[r + dr, c + dc]: the stencil flipped on both axes"""
    return np.asarray(stencil)[::-1, ::-1]


def conv_transpose(stencil, boundary, z):
    """(S^T z)[j] = sum_delta w_delta sum_{i : nb(i, delta) = j} z_i as a gather, cell by cell.  Dirichlet: i = j - delta if it is a
    cell.  Neumann: the preimages of r under the clamp are r, -1 (when r == 0) and ny (when r == ny - 1), likewise for c; i =
    preimage - delta if it is a cell."""
    ny, nx = z.shape
    w = correlation_weights(stencil)
    out = np.zeros_like(z, dtype=np.float64)
    for r in range(ny):
        for c in range(nx):
            if boundary == "neumann":
                rows = [r] + ([-1] if r == 0 else []) + ([ny] if r == ny - 1 else [])
                cols = [c] + ([-1] if c == 0 else []) + ([nx] if c == nx - 1 else [])
            else:
                rows, cols = [r], [c]
            s = 0.0
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    for pr in rows:
                        for pc in cols:
                            ir, ic = pr - dr, pc - dc
                            if 0 <= ir < ny and 0 <= ic < nx:
                                s += w[dr + 1, dc + 1] * z[ir, ic]
            out[r, c] = s
    return out


def transpose_apply(form, stencil, boundary, coef, x):
    """A^T x by the gather rule; x (ny, nx) or (2, ny, nx)"""
    c = 1.0 if coef is None else coef
    if form == "heat":
        return conv_transpose(stencil, boundary, c * x)
    a, b = x
    if form == "heat2":
        return np.stack([-conv_transpose(stencil, boundary, c * a), b])
    return np.stack([conv_transpose(stencil, boundary, c * b), a])


def field_gradient(form, stencil, boundary, L, R, ny, nx):
    """d/dcoef sum_b L_b^T A(coef) R_b, (ny, nx): sigma sum_b L_b[blk] o conv(R_b.u).  L, R (batch, n) flattened states."""
    m = ny * nx
    u = R[:, :m].reshape(-1, ny, nx)
    Lb = (L[:, m:] if form == "wave" else L[:, :m]).reshape(-1, ny, nx)
    sigma = -1.0 if form == "heat2" else 1.0
    return sigma * (Lb * conv(stencil, u, boundary)).sum(0)


def field_gradient_bound(form, stencil, boundary, L, R, ny, nx):
    """sum_b |L_b| o (|S| |R_b|), (ny, nx)"""
    m = ny * nx
    u = np.abs(R[:, :m]).reshape(-1, ny, nx)
    Lb = np.abs(L[:, m:] if form == "wave" else L[:, :m]).reshape(-1, ny, nx)
    return (Lb * conv(np.abs(stencil), u, boundary)).sum(0)


def contract_dense_gradient(form, stencil, boundary, dA, ny, nx):
    """A dense cotangent dA (n, n) of A(coef) -> the cotangent of the field: d coef_i = sigma sum_j dA[blk + i, j] S[i, j]"""
    m = ny * nx
    S = conv_matrix(stencil, boundary, ny, nx)
    rows = slice(m, 2 * m) if form == "wave" else slice(0, m)
    sigma = -1.0 if form == "heat2" else 1.0
    return sigma * (dA[rows, :m] * S).sum(1).reshape(ny, nx)


def assemble(form, S, coef):
    """The matrix of a block form from the (ny nx, ny nx) matrix S of the convolution and the field: what dense_matrix builds
    column by column (tests/test_stencil_host.py holds the two against each other), without the n applications."""
    m = S.shape[0]
    cS = S if coef is None else np.asarray(coef, dtype=np.float64).reshape(-1, 1) * S
    if form == "heat":
        return cS
    A = np.zeros((2 * m, 2 * m))
    eye = np.arange(m)
    if form == "heat2":
        A[:m, :m] = -cS
        A[m + eye, m + eye] = 1.0
    else:
        A[eye, m + eye] = 1.0
        A[m:, :m] = cS
    return A


@functools.lru_cache(maxsize=None)
def _cached_conv(stencil_key, boundary, ny, nx):
    S = conv_matrix(np.array(stencil_key).reshape(3, 3), boundary, ny, nx)
    S.setflags(write=False)
    return S


def cached_matrices(form, stencil, boundary, coef, ny, nx):
    """(A, the matrix of the absolute weights and field); the convolution matrices are computed once per (stencil, boundary, grid)"""
    stencil = np.asarray(stencil, dtype=np.float64)
    S = _cached_conv(tuple(float(v) for v in stencil.reshape(-1)), boundary, ny, nx)
    Sabs = _cached_conv(tuple(float(v) for v in np.abs(stencil).reshape(-1)), boundary, ny, nx)
    return assemble(form, S, coef), np.abs(assemble(form, Sabs, None if coef is None else np.abs(coef)))
