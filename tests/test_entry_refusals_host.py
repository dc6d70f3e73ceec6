"""What the C entry points of libmfx refuse, and with which code and text (no GPU): for every ``extern "C"`` function that takes a
dtype or an operator,
  (a) "dtype": dtype 7,
  (b) "null": the first pointer of the signature NULL,
  (c) "grid": p = 65536 where the entry has a grid limit of 65535,
  (d) "ws": a workspace one byte shorter than the matching *_workspace_bytes query answers (n = 64, k = 2, p = 1, d = 2, rank 1),
  (e) "ws0": ws_bytes = 0, for the entries whose size query adds slack, so that one byte less is still enough for them (the PCG
      family, mfx_precond_apply, mfx_partial_cholesky, the cross-covariance entries, mfx_gram_block).
The order of an entry's checks, and so which fault it names, is part of the C-ABI; EXPECTED pins it.  Every pointer is fake and
ws_bytes is huge where the case does not say otherwise, as in test_operator_kinds_host.py: a call that got as far as a launch would not
come back with the refusal asserted here.  Only the cases of EXPECTED are ever called.  Not in the table: (a) of mfx_gram_cross_apply
and mfx_partial_cholesky, which the library this table was recorded on ran as fp64 (they are refused now, as with_dtype refuses)."""

import ctypes

import pytest

from matfree_extensions import _lib

N, K, D, M = 64, 2, 2, 64
F = ctypes.c_void_p(64)  # never dereferenced
BIG = 1 << 40
F64 = _lib.MFX_F64
ref = ctypes.byref


def _dense(dt):
    d = _lib.Operator()
    d.kind, d.dtype, d.n, d.dense_a, d.lda = _lib.OP_DENSE, dt, N, 64, N
    return d


def _gram(dt):
    d = _lib.Operator()
    d.kind, d.dtype, d.n = _lib.OP_RBF, dt, N
    d.x = d.lengthscale = d.outputscale = d.noise = 64
    d.d, d.kernel_fn = D, _lib.KERNEL_RBF
    return d


def _net():
    net = _lib.GgnNet()  # one layer 7 -> 8: 64 parameters
    net.nlayers, net.loss, net.nsamples = 1, _lib.GGN_MSE, 9
    net.width[0], net.width[1] = 7, 8
    net.theta = net.act[0] = 64
    return net


def _comm():
    cm = _lib.Comm()
    cm.rank, cm.world, cm.nloc = 0, 1, N
    cm.allreduce_sum = _lib.ALLREDUCE_T(lambda *a: 0)
    cm.allgather = _lib.ALLGATHER_T(lambda *a: 0)
    return cm


def _tableau():
    tab = _lib.RkTableau()  # Heun
    tab.stages = 2
    tab.a[1][0] = 1.0
    tab.b[0] = tab.b[1] = 0.5
    return tab


NET, COMM, TAB = _net(), _comm(), _tableau()
DTS = (ctypes.c_double * 2)(0.1, 0.1)
GRADS = _lib.OpGrads()
G = ref(GRADS)


def _opref(make, dt, first):
    """the operator argument: NULL when the first pointer of the signature is asked to be NULL"""
    return ref(make(dt)) if first is not None else None


def _netref(first):
    return ref(NET) if first is not None else None


# name -> (call(lib, dt, first, p, wsb), size query(lib) or None).  `first` is F or None: the first pointer of the signature.
ENTRIES = {
    "mfx_op_apply": (lambda L, dt, a, p, w: L.mfx_op_apply(_opref(_dense, dt, a), F, N, F, N, p, 0, F, w, None), None),
    "mfx_op_vjp_params": (lambda L, dt, a, p, w: L.mfx_op_vjp_params(_opref(_dense, dt, a), F, N, F, N, p, G, F, w, None), None),
    "mfx_arnoldi_forward": (lambda L, dt, a, p, w: L.mfx_arnoldi_forward(_opref(_dense, dt, a), F, N, K, p, 1, F, F, F, F, F, w, None),
                            lambda L: L.mfx_workspace_bytes(ref(_dense(F64)), N, K, 1)),
    # the operator is the real form (size 2 n) of a complex-linear map on n = 32
    "mfx_arnoldi_forward_complex": (
        lambda L, dt, a, p, w: L.mfx_arnoldi_forward_complex(_opref(_dense, dt, a), F, N // 2, K, p, 1, F, F, F, F, F, w, None),
        lambda L: L.mfx_complex_workspace_bytes(ref(_dense(F64)), N // 2, K, 1)),
    "mfx_arnoldi_adjoint": (
        lambda L, dt, a, p, w: L.mfx_arnoldi_adjoint(_opref(_dense, dt, a), N, K, p, F, F, F, F, F, F, F, F, _lib.REORTHO_NONE, F, F, G, F, w,
                                                     None),
        lambda L: L.mfx_workspace_bytes(ref(_dense(F64)), N, K, 1)),
    "mfx_arnoldi_forward_sharded": (
        lambda L, dt, a, p, w: L.mfx_arnoldi_forward_sharded(_opref(_dense, dt, a), ref(COMM), F, N, K, p, 1, F, F, F, F, F, F, w, None),
        lambda L: L.mfx_sharded_workspace_bytes(ref(_dense(F64)), ref(COMM), N, K, 1)),
    "mfx_arnoldi_adjoint_sharded": (
        lambda L, dt, a, p, w: L.mfx_arnoldi_adjoint_sharded(_opref(_dense, dt, a), ref(COMM), N, K, p, F, F, F, F, F, F, F, F, F,
                                                             _lib.REORTHO_NONE, F, F, G, F, w, None),
        lambda L: L.mfx_sharded_workspace_bytes(ref(_dense(F64)), ref(COMM), N, K, 1)),
    "mfx_lanczos_forward_sharded": (
        lambda L, dt, a, p, w: L.mfx_lanczos_forward_sharded(_opref(_dense, dt, a), ref(COMM), F, N, K, p, F, F, F, F, F, w, None),
        lambda L: L.mfx_sharded_workspace_bytes(ref(_dense(F64)), ref(COMM), N, K, 1)),
    "mfx_lanczos_adjoint_sharded": (
        lambda L, dt, a, p, w: L.mfx_lanczos_adjoint_sharded(_opref(_dense, dt, a), ref(COMM), N, K, p, F, F, F, F, F, F, F, F, F, F, G, F, w,
                                                             None),
        lambda L: L.mfx_sharded_workspace_bytes(ref(_dense(F64)), ref(COMM), N, K, 1)),
    "mfx_lanczos_forward": (lambda L, dt, a, p, w: L.mfx_lanczos_forward(_opref(_dense, dt, a), F, N, K, p, F, F, F, F, F, w, None),
                            lambda L: L.mfx_workspace_bytes(ref(_dense(F64)), N, K, 1)),
    "mfx_lanczos_adjoint": (
        lambda L, dt, a, p, w: L.mfx_lanczos_adjoint(_opref(_dense, dt, a), N, K, p, F, F, F, F, F, F, F, F, F, G, F, w, None),
        lambda L: L.mfx_workspace_bytes(ref(_dense(F64)), N, K, 1)),
    "mfx_tridiag_eigh": (lambda L, dt, a, p, w: L.mfx_tridiag_eigh(a, F, K, p, K, dt, F, F, None), None),
    "mfx_slq_quadform_bwd": (lambda L, dt, a, p, w: L.mfx_slq_quadform_bwd(a, F, F, F, F, p, K, dt, F, F, K, None), None),
    "mfx_funm_coeffs": (lambda L, dt, a, p, w: L.mfx_funm_coeffs(a, F, F, F, p, K, dt, F, None), None),
    "mfx_funm_coeffs_bwd": (lambda L, dt, a, p, w: L.mfx_funm_coeffs_bwd(a, F, F, F, F, F, p, K, dt, F, F, K, F, None), None),
    "mfx_basis_combine": (lambda L, dt, a, p, w: L.mfx_basis_combine(a, F, N, K, p, dt, F, None), None),
    "mfx_basis_combine_bwd": (lambda L, dt, a, p, w: L.mfx_basis_combine_bwd(a, F, F, N, K, p, dt, F, F, F, w, None),
                              lambda L: L.mfx_basis_combine_workspace_bytes(N, K, 1, F64)),
    "mfx_rademacher": (lambda L, dt, a, p, w: L.mfx_rademacher(7, 0, p, N, dt, a, None), None),
    "mfx_pcg_solve": (
        lambda L, dt, a, p, w: L.mfx_pcg_solve(_opref(_dense, dt, a), F, N, N, p, F, 1, F, F, 3, 0, 0.0, 0.0, 0, F, F, None, F, w, None),
        lambda L: L.mfx_pcg_workspace_bytes(ref(_dense(F64)), N, 1, 1)),
    "mfx_mbcg_solve": (
        lambda L, dt, a, p, w: L.mfx_mbcg_solve(_opref(_dense, dt, a), F, N, N, p, F, 1, F, F, 3, 0, 0.0, 0.0, 0, F, F, None, None, F, F, F,
                                                F, F, w, None),
        lambda L: L.mfx_mbcg_workspace_bytes(ref(_dense(F64)), N, 1, 1, 3)),
    "mfx_pcg_solve_sharded": (
        lambda L, dt, a, p, w: L.mfx_pcg_solve_sharded(_opref(_dense, dt, a), ref(COMM), F, N, N, p, F, 1, F, F, 3, 0, 0.0, 0.0, 0, F, F,
                                                       None, F, w, None),
        lambda L: L.mfx_pcg_sharded_workspace_bytes(ref(_dense(F64)), ref(COMM), N, 1, 1)),
    "mfx_pcg_solve_reortho": (
        lambda L, dt, a, p, w: L.mfx_pcg_solve_reortho(_opref(_dense, dt, a), F, N, N, p, F, 1, F, F, 3, F, F, F, F, w, None),
        lambda L: L.mfx_pcg_workspace_bytes(ref(_dense(F64)), N, 1, 3)),
    "mfx_precond_apply": (lambda L, dt, a, p, w: L.mfx_precond_apply(dt, N, 1, a, F, F, F, N, F, N, p, F, w, None),
                          lambda L: L.mfx_pcg_workspace_bytes(ref(_dense(F64)), N, 1, 1)),
    "mfx_lowrank_apply": (lambda L, dt, a, p, w: L.mfx_lowrank_apply(dt, N, 1, a, F, F, F, N, F, N, p, F, w, None),
                          lambda L: L.mfx_lowrank_workspace_bytes(F64, N, 1, 1)),
    "mfx_precond_sample": (lambda L, dt, a, p, w: L.mfx_precond_sample(dt, N, 1, a, F, 7, 0, p, F, None), None),
    "mfx_partial_cholesky": (lambda L, dt, a, p, w: L.mfx_partial_cholesky(_opref(_gram, dt, a), 1, 1, 1, F, F, F, F, w, None),
                             lambda L: L.mfx_pcg_workspace_bytes(ref(_gram(F64)), N, 1, 1)),
    "mfx_gram_cross_apply": (lambda L, dt, a, p, w: L.mfx_gram_cross_apply(_opref(_gram, dt, a), F, M, F, N, F, M, p, F, w, None),
                             lambda L: L.mfx_gram_cross_workspace_bytes(ref(_gram(F64)), M)),
    "mfx_gram_cross_apply_t": (lambda L, dt, a, p, w: L.mfx_gram_cross_apply_t(_opref(_gram, dt, a), F, M, F, M, F, N, p, F, w, None),
                               lambda L: L.mfx_gram_cross_workspace_bytes(ref(_gram(F64)), M)),
    "mfx_gram_cross_vjp": (lambda L, dt, a, p, w: L.mfx_gram_cross_vjp(_opref(_gram, dt, a), F, M, F, M, F, N, p, G, F, F, w, None),
                           lambda L: L.mfx_gram_cross_vjp_workspace_bytes(ref(_gram(F64)), M, 1)),
    "mfx_gram_cross_vjp_dense": (lambda L, dt, a, p, w: L.mfx_gram_cross_vjp_dense(_opref(_gram, dt, a), F, M, F, N, G, F, F, w, None),
                                 lambda L: L.mfx_gram_cross_vjp_dense_workspace_bytes(ref(_gram(F64)), M)),
    "mfx_gram_block": (lambda L, dt, a, p, w: L.mfx_gram_block(_opref(_gram, dt, a), F, M, F, M, F, M, F, w, None),
                       lambda L: L.mfx_gram_block_workspace_bytes(ref(_gram(F64)), M, M)),
    "mfx_rff_apply": (lambda L, dt, a, p, w: L.mfx_rff_apply(dt, a, D, N, D, F, F, M, F, 0, F, F, M, p, F, N, None), None),
    "mfx_rff_grad_x": (lambda L, dt, a, p, w: L.mfx_rff_grad_x(dt, a, D, N, D, F, F, M, F, 0, F, F, M, p, F, N, F, D, None), None),
    "mfx_mlp_jac_apply": (lambda L, dt, a, p, w: L.mfx_mlp_jac_apply(_netref(a), dt, F, N, p, F, None), None),
    "mfx_mlp_jac_t_apply": (lambda L, dt, a, p, w: L.mfx_mlp_jac_t_apply(_netref(a), dt, F, p, F, N, F, w, None),
                            lambda L: L.mfx_mlp_jac_workspace_bytes(ref(NET), F64, 1)),
    "mfx_ggn_diag": (lambda L, dt, a, p, w: L.mfx_ggn_diag(_netref(a), dt, F, F, w, None),
                     lambda L: L.mfx_ggn_diag_workspace_bytes(ref(NET), F64)),
    "mfx_rk_solve": (
        lambda L, dt, a, p, w: L.mfx_rk_solve(_opref(_dense, dt, a), ref(TAB), DTS, 2, F, N, N, p, F, N, None, 0, F, w, None),
        lambda L: L.mfx_rk_workspace_bytes(ref(_dense(F64)), ref(TAB), N, 1, 0)),
    "mfx_rk_adjoint": (
        lambda L, dt, a, p, w: L.mfx_rk_adjoint(_opref(_dense, dt, a), ref(TAB), DTS, 2, F, N, p, F, N, F, N, G, 0, F, w, None),
        lambda L: L.mfx_rk_workspace_bytes(ref(_dense(F64)), ref(TAB), N, 1, 1)),
    "mfx_rk_backsolve": (
        lambda L, dt, a, p, w: L.mfx_rk_backsolve(_opref(_dense, dt, a), ref(TAB), DTS, 2, F, N, N, p, F, N, F, N, G, 0, F, w, None),
        lambda L: L.mfx_rk_workspace_bytes(ref(_dense(F64)), ref(TAB), N, 1, 2)),
}


def run_case(lib, name, case):
    """-> (code, text) of one case: "dtype", "null", "grid", "ws" or "ws0" """
    call, query = ENTRIES[name]
    if case == "dtype":
        rc = call(lib, 7, F, 1, BIG)
    elif case == "null":
        rc = call(lib, F64, None, 1, BIG)
    elif case == "grid":
        rc = call(lib, F64, F, 65536, BIG)
    elif case == "ws0":
        rc = call(lib, F64, F, 1, 0)
    else:
        need = query(lib)
        assert need > 0, (name, need)
        rc = call(lib, F64, F, 1, need - 1)
    return rc, lib.mfx_last_error().decode()


# entry -> case -> (code, piece of the text): the answers of the library before the rewrite
EXPECTED = {'mfx_op_apply': {'dtype': (-2, 'unsupported dtype 7'), 'null': (-1, 'null argument'), 'grid': (-2, 'p too large')},
 'mfx_op_vjp_params': {'dtype': (-2, 'unsupported dtype 7'), 'null': (-1, 'null argument')},
 'mfx_arnoldi_forward': {'dtype': (-2, 'unsupported dtype 7'),
                         'null': (-1, 'operator is NULL'),
                         'grid': (-2, 'p=65536 exceeds the grid limit 65535'),
                         'ws': (-4, 'workspace too small')},
 'mfx_arnoldi_forward_complex': {'dtype': (-2, 'unsupported dtype 7'),
                                 'null': (-1, 'null argument'),
                                 'grid': (-2, 'p=65536 exceeds the grid limit 65535'),
                                 'ws': (-4, 'workspace too small')},
 'mfx_arnoldi_adjoint': {'dtype': (-2, 'unsupported dtype 7'),
                         'null': (-1, 'operator is NULL'),
                         'grid': (-2, 'p=65536 exceeds the grid limit 65535'),
                         'ws': (-4, 'workspace too small')},
 'mfx_arnoldi_forward_sharded': {'dtype': (-2, 'unsupported dtype 7'),
                                 'null': (-1, 'operator is NULL'),
                                 'grid': (-2, 'p=65536 exceeds the grid limit 65535'),
                                 'ws': (-4, 'workspace too small')},
 'mfx_arnoldi_adjoint_sharded': {'dtype': (-2, 'unsupported dtype 7'),
                                 'null': (-1, 'operator is NULL'),
                                 'grid': (-2, 'p=65536 exceeds the grid limit 65535'),
                                 'ws': (-4, 'workspace too small')},
 'mfx_lanczos_forward_sharded': {'dtype': (-2, 'unsupported dtype 7'),
                                 'null': (-1, 'operator is NULL'),
                                 'grid': (-2, 'p=65536 exceeds the grid limit 65535'),
                                 'ws': (-4, 'workspace too small')},
 'mfx_lanczos_adjoint_sharded': {'dtype': (-2, 'unsupported dtype 7'),
                                 'null': (-1, 'operator is NULL'),
                                 'grid': (-2, 'p=65536 exceeds the grid limit 65535'),
                                 'ws': (-4, 'workspace too small')},
 'mfx_lanczos_forward': {'dtype': (-2, 'unsupported dtype 7'),
                         'null': (-1, 'operator is NULL'),
                         'grid': (-2, 'p=65536 exceeds the grid limit 65535'),
                         'ws': (-4, 'workspace too small')},
 'mfx_lanczos_adjoint': {'dtype': (-2, 'unsupported dtype 7'),
                         'null': (-1, 'operator is NULL'),
                         'grid': (-2, 'p=65536 exceeds the grid limit 65535'),
                         'ws': (-4, 'workspace too small')},
 'mfx_tridiag_eigh': {'dtype': (-2, 'unsupported dtype 7'), 'null': (-1, 'null argument')},
 'mfx_slq_quadform_bwd': {'dtype': (-2, 'unsupported dtype 7'), 'null': (-1, 'null argument')},
 'mfx_funm_coeffs': {'dtype': (-2, 'unsupported dtype 7'), 'null': (-1, 'null argument')},
 'mfx_funm_coeffs_bwd': {'dtype': (-2, 'unsupported dtype 7'), 'null': (-1, 'null argument')},
 'mfx_basis_combine': {'dtype': (-2, 'unsupported dtype 7'),
                       'null': (-1, 'null argument'),
                       'grid': (-2, 'basis combination supports p <= 65535 vectors per call (got 65536)')},
 'mfx_basis_combine_bwd': {'dtype': (-2, 'unsupported dtype 7'),
                           'null': (-1, 'dcoeffs needs the basis'),
                           'grid': (-2, 'basis combination supports p <= 65535 vectors per call (got 65536)'),
                           'ws': (-4, 'workspace too small')},
 'mfx_rademacher': {'dtype': (-2, 'unsupported dtype 7'), 'null': (-1, 'bad argument'), 'grid': (-1, 'bad argument')},
 'mfx_pcg_solve': {'ws0': (-4, 'workspace too small'), 'dtype': (-1, 'bad dtype'), 'null': (-1, 'mfx_pcg_solve: null argument'), 'grid': (-2, 'at most 65535 right-hand sides per call')},
 'mfx_mbcg_solve': {'ws0': (-4, 'workspace too small'), 'dtype': (-1, 'bad dtype'),
                    'null': (-1, 'mfx_mbcg_solve: null argument'),
                    'grid': (-2, 'at most 65535 right-hand sides per call')},
 'mfx_pcg_solve_sharded': {'ws0': (-4, 'workspace too small'), 'dtype': (-1, 'bad dtype'),
                           'null': (-1, 'mfx_pcg_solve_sharded: null argument'),
                           'grid': (-2, 'at most 65535 right-hand sides per call')},
 'mfx_pcg_solve_reortho': {'ws0': (-4, 'workspace too small'), 'dtype': (-1, 'bad dtype'),
                           'null': (-1, 'mfx_pcg_solve_reortho: null argument'),
                           'grid': (-2, 'at most 65535 right-hand sides per call')},
 'mfx_precond_apply': {'ws0': (-4, 'workspace too small'), 'dtype': (-1, 'bad dtype'),
                       'null': (-1, 'preconditioner needs lt, minv and shift'),
                       'grid': (-2, 'at most 65535 vectors per call')},
 'mfx_lowrank_apply': {'dtype': (-2, 'mfx_lowrank_apply: unsupported dtype 7'),
                       'null': (-1, 'mfx_lowrank_apply: null factor (lt, mid or scale)'),
                       'ws': (-4, 'workspace too small')},
 'mfx_precond_sample': {'dtype': (-1, 'bad dtype'), 'null': (-1, 'mfx_precond_sample: rank > 0 needs lt and shift')},
 'mfx_partial_cholesky': {'ws0': (-4, 'workspace too small'), 'null': (-1, 'mfx_partial_cholesky: null argument')},
 'mfx_gram_cross_apply': {'ws0': (-4, 'workspace too small'), 'null': (-1, 'mfx_gram_cross_apply: null argument')},
 'mfx_gram_cross_apply_t': {'ws0': (-4, 'workspace too small'), 'dtype': (-1, 'unsupported dtype 7'), 'null': (-1, 'mfx_gram_cross_apply_t: null argument')},
 'mfx_gram_cross_vjp': {'ws0': (-4, 'workspace too small'), 'dtype': (-1, 'unsupported dtype 7'), 'null': (-1, 'mfx_gram_cross_vjp: null argument')},
 'mfx_gram_cross_vjp_dense': {'ws0': (-4, 'workspace too small'), 'dtype': (-1, 'unsupported dtype 7'), 'null': (-1, 'mfx_gram_cross_vjp_dense: null argument')},
 'mfx_gram_block': {'ws0': (-4, 'workspace too small'), 'dtype': (-1, 'unsupported dtype 7'), 'null': (-1, 'mfx_gram_block: null argument')},
 'mfx_rff_apply': {'dtype': (-1, 'mfx_rff_apply: unknown dtype 7'),
                   'null': (-1, 'mfx_rff_apply: x, omega, phase, lengthscale, outputscale and W must not be NULL')},
 'mfx_rff_grad_x': {'dtype': (-1, 'mfx_rff_grad_x: unknown dtype 7'),
                    'null': (-1, 'mfx_rff_grad_x: x, omega, phase, lengthscale, outputscale and W must not be NULL')},
 'mfx_mlp_jac_apply': {'dtype': (-2, 'MLP Jacobian: unsupported dtype 7'),
                       'null': (-1, 'MLP Jacobian: net is NULL'),
                       'grid': (-2, 'MLP Jacobian: p too large (at most 65535 vectors per call)')},
 'mfx_mlp_jac_t_apply': {'dtype': (-2, 'MLP Jacobian: unsupported dtype 7'),
                         'null': (-1, 'MLP Jacobian: net is NULL'),
                         'grid': (-2, 'MLP Jacobian: p too large (at most 65535 vectors per call)'),
                         'ws': (-4, 'workspace too small')},
 'mfx_ggn_diag': {'dtype': (-2, 'GGN diagonal: unsupported dtype 7'), 'null': (-1, 'GGN diagonal: net is NULL'), 'ws': (-4, 'workspace too small')},
 'mfx_rk_solve': {'dtype': (-2, 'unsupported dtype 7'),
                  'null': (-1, 'operator is NULL'),
                  'grid': (-2, 'p = 65536 exceeds the grid limit 65535'),
                  'ws': (-4, 'workspace too small')},
 'mfx_rk_adjoint': {'dtype': (-2, 'unsupported dtype 7'),
                    'null': (-1, 'operator is NULL'),
                    'grid': (-2, 'p = 65536 exceeds the grid limit 65535'),
                    'ws': (-4, 'workspace too small')},
 'mfx_rk_backsolve': {'dtype': (-2, 'unsupported dtype 7'),
                      'null': (-1, 'operator is NULL'),
                      'grid': (-2, 'p = 65536 exceeds the grid limit 65535'),
                      'ws': (-4, 'workspace too small')}}


def _cases():
    return [(name, case) for name, table in EXPECTED.items() for case in table]


def test_the_table_names_every_entry_point():
    assert set(EXPECTED) == set(ENTRIES)
    assert len(_cases()) == sum(len(t) for t in EXPECTED.values())


@pytest.mark.parametrize("name,case", _cases(), ids=[f"{n}-{c}" for n, c in _cases()])
def test_entry_point_refuses_as_before(name, case):
    lib = _lib.get()
    code, text = EXPECTED[name][case]
    got, said = run_case(lib, name, case)
    assert got == code and text in said, (name, case, got, said)
