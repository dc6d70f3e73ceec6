"""NumPy fp64 restatement of the affine vector field y' = A y + b and of its bordered linear form B = [[A, b], [0, 0]] on (y, 1):
the yardstick of tests/test_affine_host.py and tests/test_gpu_affine.py.

  bordered       the dense (m + 1, m + 1) matrix from a dense A and b
  stencil_dense  A of a stencil system, column by column (tests/_stencil_restatement.py)
  expm           scipy.linalg.expm when SciPy imports, else scaling and squaring of a Taylor series
  phi1_times     phi_1(A) b = sum_k A^k b / (k + 1)!, the series itself: independent of expm and of the border
  rk_affine      the explicit Runge-Kutta loop written on y' = A y + b -- NOT on the bordered system, so that a comparison with
                 rk_linear on B checks the stage-by-stage equivalence instead of assuming it
  rk_linear      the same loop on a linear field z' = B z

States are rows: y (p, m)."""

import numpy as np

import _stencil_restatement as sr


def bordered(A, b):
    m = A.shape[0]
    B = np.zeros((m + 1, m + 1))
    B[:m, :m] = A
    B[:m, m] = np.asarray(b, dtype=np.float64).reshape(m)
    return B


def stencil_dense(form, stencil, boundary, coef, ny, nx):
    return sr.dense_matrix(form, np.asarray(stencil, dtype=np.float64), boundary, coef, ny, nx)


def lift(y):
    return np.concatenate([y, np.ones(y.shape[:-1] + (1,))], axis=-1)


def expm(M):
    try:
        import scipy.linalg

        return scipy.linalg.expm(M)
    except ImportError:
        squarings = max(0, int(np.ceil(np.log2(max(np.abs(M).sum(1).max(), 1e-300)))) + 4)
        X = M / 2.0**squarings
        out, term = np.eye(M.shape[0]), np.eye(M.shape[0])
        for k in range(1, 30):
            term = term @ X / k
            out = out + term
        for _ in range(squarings):
            out = out @ out
        return out


def phi1_times(A, b, terms=60):
    """phi_1(A) b by its power series (small |A| only)"""
    out, term = np.zeros_like(b, dtype=np.float64), np.asarray(b, dtype=np.float64)
    for k in range(terms):
        term = term if k == 0 else A @ term / (k + 1)  # A^k b / (k + 1)!
        out = out + term
    return out


def _tableau(tab):
    s = len(tab.b)
    a = np.zeros((s, s))
    for i, row in enumerate(tab.a):
        a[i, : len(row)] = [float(v) for v in row]
    return a, np.array([float(v) for v in tab.b])


def _rk(field, y0, tab, dts):
    a, b = _tableau(tab)
    y = np.asarray(y0, dtype=np.float64)
    for h in dts:
        Ks = []
        for i in range(len(b)):
            Y = y + sum(float(h) * a[i, j] * Ks[j] for j in range(i) if a[i, j] != 0.0)
            Ks.append(field(Y))
        y = y + sum(float(h) * b[i] * Ks[i] for i in range(len(b)) if b[i] != 0.0)
    return y


def rk_affine(A, b, y0, tab, dts):
    return _rk(lambda Y: Y @ A.T + b.reshape(1, -1), y0, tab, dts)


def rk_linear(B, z0, tab, dts):
    return _rk(lambda Z: Z @ B.T, z0, tab, dts)
