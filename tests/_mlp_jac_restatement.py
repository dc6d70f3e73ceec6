"""NumPy fp64 restatement of the two Jacobian maps of an MLP, written from the formulas of include/mfx.h (next to struct mfx_ggn_net),
not from the kernels: per sample i, in theta's layout (per layer the bias, then the kernel (w_{l-1}, w_l) row-major)

    J V:    t_0 = 0;  s_l = V_W_l^T a_{l-1} + v_b_l + W_l^T t_{l-1};  t_l = dact_l o s_l (l < L);  out[b][i] = t_L = s_L
    J^T U:  g_L = u_bi;  y_b_l += g_l;  y_W_l += a_{l-1} g_l^T;  g_{l-1} = dact_{l-1} o (W_l g_l);  y_b = sum_i (.)

The tape is the one of tests/_ggn_restatement.py (``tape``), whose ``split`` and ``param_count`` are used here.  Plain helper module
(no tests): tests/test_mlp_jac_host.py ties it to torch.func, tests/test_gpu_mlp_jac.py measures the kernels against it.
"""

import numpy as np

from _ggn_restatement import param_count, split


def _forward(tp, theta, widths, V, absolute):
    f = np.abs if absolute else (lambda t: t)
    V = np.asarray(V, dtype=np.float64)
    assert V.ndim == 2 and V.shape[1] == param_count(widths)
    layers = split(f(np.asarray(theta, dtype=np.float64)), widths)
    vl = split(f(V), widths)
    L = len(layers)
    t = None
    for l in range(1, L + 1):
        (vb, vW), (_, W) = vl[l - 1], layers[l - 1]
        s = np.einsum("nk,bkj->bnj", f(tp["act"][l - 1]), vW) + vb[:, None, :]
        if t is not None:
            s = s + np.einsum("bnk,kj->bnj", t, W)
        t = f(tp["dact"][l])[None] * s if l < L else s
    return t


def _backward(tp, theta, widths, U, absolute):
    f = np.abs if absolute else (lambda t: t)
    g = f(np.asarray(U, dtype=np.float64))
    n = tp["act"][0].shape[0]
    assert g.ndim == 3 and g.shape[1:] == (n, widths[-1])
    layers = split(f(np.asarray(theta, dtype=np.float64)), widths)
    L = len(layers)
    out = np.zeros((g.shape[0], param_count(widths)))
    off = [0]
    for wi, wo in zip(widths[:-1], widths[1:]):
        off.append(off[-1] + (wi + 1) * wo)
    for l in range(L, 0, -1):
        wi, wo = widths[l - 1], widths[l]
        out[:, off[l - 1] : off[l - 1] + wo] = g.sum(1)
        out[:, off[l - 1] + wo : off[l]] = np.einsum("nk,bnj->bkj", f(tp["act"][l - 1]), g).reshape(len(g), wi * wo)
        if l > 1:
            g = f(tp["dact"][l - 1])[None] * np.einsum("bnj,kj->bnk", g, layers[l - 1][1])
    return out


def jac_apply_from_tape(tp, theta, widths, V):
    """(p, P) -> (p, N, c): J v for every row v of V"""
    return _forward(tp, theta, widths, V, False)


def abs_jac_apply_from_tape(tp, theta, widths, V):
    """the scale |J| |v|: the same chain with every operand replaced by its absolute value"""
    return _forward(tp, theta, widths, V, True)


def jac_t_apply_from_tape(tp, theta, widths, U):
    """(p, N, c) -> (p, P): J^T u for every u of U"""
    return _backward(tp, theta, widths, U, False)


def abs_jac_t_apply_from_tape(tp, theta, widths, U):
    """the scale |J|^T |u|"""
    return _backward(tp, theta, widths, U, True)


def dense_jacobian(tp, theta, widths):
    """J as an (N, c, P) array: J applied to the identity (row b of the result is the column J e_b)"""
    return np.moveaxis(jac_apply_from_tape(tp, theta, widths, np.eye(param_count(widths))), 0, -1)
