"""NumPy fp64 restatement of the GGN operator of an MLP, written from the formulas of include/mfx.h (struct mfx_ggn_net), not from the
kernel: per sample i and vector v, in theta's layout (per layer the bias, then the kernel (w_{l-1}, w_l) row-major)

    t_0 = 0;  s_l = V_W_l^T a_{l-1} + v_b_l + W_l^T t_{l-1};  t_l = dact_l o s_l (l < L),  t_L = s_L
    u = p o t_L - p (p . t_L)   (cross-entropy)      u = t_L   (mse)
    g_L = u;  y_b_l += g_l;  y_W_l += a_{l-1} g_l^T;  g_{l-1} = dact_{l-1} o (W_l g_l);      y = sum_i (.) + alpha v

Plain helper module (no tests): tests/test_ggn_host.py ties it to torch.func, tests/test_gpu_ggn.py measures the kernels against it.
"""

import numpy as np

LOSSES = ("cross_entropy", "mse")
ACTIVATIONS = ("tanh", "relu")


def param_count(widths):
    return sum((wi + 1) * wo for wi, wo in zip(widths[:-1], widths[1:]))


def split(vec, widths):
    """(..., P) -> [(bias (..., w_l), kernel (..., w_{l-1}, w_l))] for l = 1..L"""
    out, off = [], 0
    for wi, wo in zip(widths[:-1], widths[1:]):
        out.append((vec[..., off : off + wo], vec[..., off + wo : off + wo + wi * wo].reshape(*vec.shape[:-1], wi, wo)))
        off += (wi + 1) * wo
    assert off == vec.shape[-1]
    return out


def tape(theta, x, widths, activation, loss="cross_entropy"):
    """{"act": [a_0 = x, ..., a_{L-1}], "dact": [None, phi'(z_1), ...], "logits", "prob" (None for mse)}, all fp64"""
    a = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    layers = split(np.asarray(theta, dtype=np.float64), widths)
    act, dact = [a], [None]
    for l, (b, W) in enumerate(layers, start=1):
        z = a @ W + b
        if l < len(layers):
            if activation == "tanh":
                a = np.tanh(z)
                d = 1.0 - a * a
            else:
                a = np.maximum(z, 0.0)
                d = (z > 0).astype(np.float64)
            act.append(a)
            dact.append(d)
    prob = None
    if loss == "cross_entropy":
        e = np.exp(z - z.max(-1, keepdims=True))
        prob = e / e.sum(-1, keepdims=True)
    return {"act": act, "dact": dact, "logits": z, "prob": prob}


def _chain(tp, theta, widths, V, alpha, loss, absolute):
    f = np.abs if absolute else (lambda t: t)
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    layers = split(f(np.asarray(theta, dtype=np.float64)), widths)
    vl = split(f(V), widths)
    L = len(layers)
    act = [f(a) for a in tp["act"]]
    dact = [None] + [f(d) for d in tp["dact"][1:]]
    t = None
    for l in range(1, L + 1):
        (vb, vW), (_, W) = vl[l - 1], layers[l - 1]
        s = np.einsum("nk,bkj->bnj", act[l - 1], vW) + vb[:, None, :]
        if t is not None:
            s = s + np.einsum("bnk,kj->bnj", t, W)
        t = dact[l][None] * s if l < L else s
    if loss == "cross_entropy":
        p = f(tp["prob"])[None]
        dot = (p * t).sum(-1, keepdims=True)
        g = p * t + p * dot if absolute else p * t - p * dot
    else:
        g = t
    out = np.zeros_like(V)
    off = [0]
    for wi, wo in zip(widths[:-1], widths[1:]):
        off.append(off[-1] + (wi + 1) * wo)
    for l in range(L, 0, -1):
        wi, wo = widths[l - 1], widths[l]
        out[:, off[l - 1] : off[l - 1] + wo] = g.sum(1)
        out[:, off[l - 1] + wo : off[l]] = np.einsum("nk,bnj->bkj", act[l - 1], g).reshape(len(V), wi * wo)
        if l > 1:
            g = dact[l - 1][None] * np.einsum("bnj,kj->bnk", g, layers[l - 1][1])
    return out + f(np.float64(alpha)) * f(V)


def apply_from_tape(tp, theta, widths, V, alpha, loss="cross_entropy"):
    """(p, P) -> (p, P): A(alpha) v for every row v of V"""
    return _chain(tp, theta, widths, V, alpha, loss, False)


def abs_apply_from_tape(tp, theta, widths, V, alpha, loss="cross_entropy"):
    """the scale s = |A| |v|: the same chain with every operand replaced by its absolute value and |H| = diag(p) + p p^T"""
    return _chain(tp, theta, widths, V, alpha, loss, True)


def dense_matrix(tp, theta, widths, alpha, loss="cross_entropy"):
    """A(alpha) as a (P, P) matrix: the operator applied to the identity (row b = A e_b; A is symmetric)"""
    return apply_from_tape(tp, theta, widths, np.eye(param_count(widths)), alpha, loss)
