"""NumPy fp64 restatement of the exact GGN diagonal of an MLP, written from the formulas of include/mfx.h (at mfx_ggn_diag), not from
the kernel.  For sample i and class o, g_L = e_o and g_{l-1} = dact_{l-1} o (W_l g_l); per sample, layer and unit

    D[m] = max(sum_o p_o g_m^2 - (sum_o p_o g_m)^2, 0)   (cross-entropy)        D[m] = sum_o g_m^2   (mse)
    diag[bias (l, m)] = sum_i D_il[m]        diag[kernel (l, k, m)] = sum_i a_{i,l-1,k}^2 D_il[m]

in theta's layout.  Tapes have the format of tests/_ggn_restatement.py::tape.  Plain helper module (no tests):
tests/test_ggn_diag_host.py ties it to the dense matrix and to torch.func, tests/test_gpu_ggn_diag.py measures the kernel against it.
"""

import numpy as np

import _ggn_restatement as gr


def _chain(tp, theta, widths, loss, absolute):
    f = np.abs if absolute else (lambda t: t)
    layers = gr.split(f(np.asarray(theta, dtype=np.float64)), widths)
    L, c = len(layers), widths[-1]
    act = [f(np.asarray(a, dtype=np.float64)) for a in tp["act"]]
    dact = [None] + [f(np.asarray(d, dtype=np.float64)) for d in tp["dact"][1:]]
    N = act[0].shape[0]
    g = np.broadcast_to(np.eye(c), (N, c, c)).copy()  # g[i, o, m]: row o of J_i at the units m of the layer at hand
    out = np.zeros(gr.param_count(widths))
    off = [0]
    for wi, wo in zip(widths[:-1], widths[1:]):
        off.append(off[-1] + (wi + 1) * wo)
    for l in range(L, 0, -1):
        wi, wo = widths[l - 1], widths[l]
        if loss == "cross_entropy":
            p = f(np.asarray(tp["prob"], dtype=np.float64))
            m1, m2 = np.einsum("no,nom->nm", p, g * g), np.einsum("no,nom->nm", p, g)
            D = m1 + m2 * m2 if absolute else np.maximum(m1 - m2 * m2, 0.0)
        else:
            D = (g * g).sum(1)
        out[off[l - 1] : off[l - 1] + wo] = D.sum(0)
        out[off[l - 1] + wo : off[l]] = np.einsum("nk,nm->km", act[l - 1] ** 2, D).reshape(wi * wo)
        if l > 1:
            g = dact[l - 1][:, None, :] * np.einsum("nom,km->nok", g, layers[l - 1][1])
    return out


def diag_from_tape(tp, theta, widths, loss="cross_entropy"):
    """(P,): sum_i diag(J_i^T H_i J_i), the clamp included"""
    return _chain(tp, theta, widths, loss, False)


def abs_diag_from_tape(tp, theta, widths, loss="cross_entropy"):
    """the scale s: the same chain with every operand replaced by its absolute value and the subtraction by an addition
    (cross-entropy: D_abs = sum p g_abs^2 + (sum p g_abs)^2)"""
    return _chain(tp, theta, widths, loss, True)


def hutchinson_recursion(A, draws):
    """bnn_baselines.hutchinson_diagonal written out: draws (levels, samples, P), A (P, P) applied as eps -> A eps"""
    diag = np.zeros(draws.shape[-1])
    for n, eps in enumerate(draws):
        update = np.mean([e * (A @ e - diag * e) for e in eps], axis=0) + diag
        diag = (diag * n + update) / (n + 1)
    return diag
