"""NumPy restatement of the adaptive-step Runge-Kutta solve of y' = A y (csrc/mfx_rk.hip, mfx_rk_solve_adaptive) on a DENSE matrix:
the yardstick of tests/test_rk_adaptive_host.py and tests/test_gpu_rk_adaptive.py.

The scheme is the fixed-step one of tests/_rk_restatement.py with every stage of the pair's tableau evaluated (dopri5: seven, the
last at Y_7 = y + h sum_j a_7j K_j, which is y+ up to rounding; no first-same-as-last reuse).  The controller is written from
scipy 1.15's ``RungeKutta._step_impl``:

    t+ = min(t + H, t1), h = t+ - t;   err = h sum_i e_i K_i;   scale = atol + rtol max(|y|, |y+|)
    norm = max over the states of sqrt(mean (err / scale)^2)       -- the batch shares one step sequence
    norm < 1:  accept, H <- h f,  f = 10 if norm == 0 else min(10, 0.9 norm^(-1/order)), at most 1 after a rejection
    else:      reject, H <- h max(0.2, 0.9 norm^(-1/order))

``dtype``: the format of the states, the stage values, A and the coefficients h a_ij (fp64 products rounded once), as on the device;
the error estimate, the scale and the norm are fp64 arithmetic on those stored values in either case."""

import numpy as np

OK, MAX_ATTEMPTS, STEP_TOO_SMALL, NONFINITE = 0, 1, 2, 3


def full_pair(pair):
    """(a (s, s) strictly lower, b (s,), e (s,)) as fp64 arrays from a rk_tableaux.Pair"""
    s = len(pair.tab.b)
    a = np.zeros((s, s))
    for i, row in enumerate(pair.tab.a):
        a[i, : len(row)] = row
    return a, np.array(pair.tab.b, dtype=np.float64), np.array(pair.e, dtype=np.float64)


def heat_matrix(ny, nx, dx, c=1.0):
    """c x the 5-point Laplacian / dx^2 with a Dirichlet boundary on the row-major flattened (ny, nx) grid"""
    def second(m):
        return -2.0 * np.eye(m) + np.eye(m, k=1) + np.eye(m, k=-1)

    return c * (np.kron(second(ny), np.eye(nx)) + np.kron(np.eye(ny), second(nx))) / dx**2


def attempt(A, y, a, b, e, h, dtype):
    """one step of size h from the rows y -> (y+, err in fp64)"""
    s = len(b)
    K = []
    for i in range(s):
        Y = y
        for j in range(i):
            c = dtype(h * a[i, j])
            if c != 0:
                Y = Y + c * K[j]
        K.append((Y @ A.T).astype(dtype))
    ynew = y
    for i in range(s):
        c = dtype(h * b[i])
        if c != 0:
            ynew = ynew + c * K[i]
    err = np.zeros(y.shape, dtype=np.float64)
    for i in range(s):
        if e[i] != 0.0:
            err = err + (h * e[i]) * K[i].astype(np.float64)
    return ynew.astype(dtype), err


def solve(A, y0, pair, t0, t1, dt0, rtol, atol, max_attempts=100000, dtype=np.float64):
    """-> dict(status, ts, dts, n_accepted, n_rejected, norms (every attempt's, in order), y1 (p, n), ys (p, n_accepted + 1, n))"""
    a, b, e = full_pair(pair)
    A = np.asarray(A).astype(dtype)
    y = np.atleast_2d(np.asarray(y0)).astype(dtype)
    expo = -1.0 / pair.order
    t, h_abs = float(t0), float(dt0)
    ts, dts, norms, ys = [t], [], [], [y]
    status, rejected, n_rejected, attempts = OK, False, 0, 0
    while t < t1:
        if attempts >= max_attempts:
            status = MAX_ATTEMPTS
            break
        if h_abs < 10.0 * (np.nextafter(t, np.inf) - t):
            status = STEP_TOO_SMALL
            break
        t_new = min(t + h_abs, t1)
        h = t_new - t
        ynew, err = attempt(A, y, a, b, e, h, dtype)
        attempts += 1
        scale = atol + rtol * np.maximum(np.abs(y.astype(np.float64)), np.abs(ynew.astype(np.float64)))
        sums = ((err / scale) ** 2).sum(axis=1)
        if not np.all(np.isfinite(sums)):
            status = NONFINITE
            break
        norm = float(np.sqrt(sums.max() / y.shape[1]))
        norms.append(norm)
        if norm < 1.0:
            factor = 10.0 if norm == 0.0 else min(10.0, 0.9 * norm**expo)
            if rejected:
                factor = min(1.0, factor)
            t, y, h_abs, rejected = t_new, ynew, h * factor, False
            ts.append(t)
            dts.append(h)
            ys.append(y)
        else:
            h_abs, rejected = h * max(0.2, 0.9 * norm**expo), True
            n_rejected += 1
    return {"status": status, "ts": np.array(ts), "dts": np.array(dts), "n_accepted": len(dts), "n_rejected": n_rejected,
            "norms": np.array(norms), "y1": y, "ys": np.stack(ys, axis=1)}


def clear_of_ties(res, margin=0.01):
    """no accept / reject decision of the solve lies within `margin` of norm == 1: a condition on the INPUTS of a parity test"""
    return bool(np.all(np.abs(res["norms"] - 1.0) > margin))
