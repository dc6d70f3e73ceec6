"""CPU-side checks of the reverse mode of the cross-covariance matvec (no GPU): the three C-ABI entry points are declared,
mirrored in ctypes and exported, and every refusal comes back with its code and message before any launch."""

import ctypes
import os

import pytest

from matfree_extensions import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfx_gram_cross_apply_t", "mfx_gram_cross_vjp_workspace_bytes", "mfx_gram_cross_vjp")
FAKE = ctypes.c_void_p(64)  # a device pointer no kernel may touch: every call below must return before a launch
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


def test_new_symbols_are_declared_mirrored_and_exported():
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    lib = _lib.get()
    for name in NEW:
        assert f" {name}(" in header, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None


def _rbf(n=300, d=3, nrows=0, dtype=_lib.MFX_F32):
    desc = _lib.Operator()
    desc.kind, desc.dtype, desc.n = _lib.OP_RBF, dtype, n
    desc.x = desc.lengthscale = desc.outputscale = desc.noise = 64
    desc.d, desc.ard = d, 0
    desc.row0, desc.nrows = 0, nrows
    return desc


def _grads(**fields):
    g = _lib.OpGrads()
    for k, v in fields.items():
        setattr(g, k, v)
    return g


def _vjp(desc, m=7, ldl=7, ldr=None, batch=2, grads=None, ws_bytes=1 << 30, ws=FAKE, xnew=FAKE):
    ldr = desc.n if ldr is None else ldr
    grads = _grads(lengthscale=64, outputscale=64, x=64) if grads is None else grads
    return _lib.get().mfx_gram_cross_vjp(ctypes.byref(desc), xnew, m, FAKE, ldl, FAKE, ldr, batch, ctypes.byref(grads), FAKE, ws,
                                          ws_bytes, None)


def _apply_t(desc, m=7, ldu=7, ldy=None, p=2, ws_bytes=1 << 30, ws=FAKE, u=FAKE):
    ldy = desc.n if ldy is None else ldy
    return _lib.get().mfx_gram_cross_apply_t(ctypes.byref(desc), FAKE, m, u, ldu, FAKE, ldy, p, ws, ws_bytes, None)


def _err():
    return _lib.get().mfx_last_error().decode()


def test_workspace_queries():
    lib = _lib.get()
    desc = _rbf()
    need = lib.mfx_gram_cross_vjp_workspace_bytes(ctypes.byref(desc), 16, 3)
    assert need >= lib.mfx_gram_cross_workspace_bytes(ctypes.byref(desc), 16) > 0
    dense = _lib.Operator()
    dense.kind, dense.dtype, dense.n = _lib.OP_DENSE, _lib.MFX_F32, 4
    assert lib.mfx_gram_cross_vjp_workspace_bytes(ctypes.byref(dense), 16, 3) == -1
    assert lib.mfx_gram_cross_vjp_workspace_bytes(ctypes.byref(desc), 0, 3) == -1
    # a small owner set against many columns: the per-split partials are part of the size
    big = _rbf(n=131072, d=8)
    assert lib.mfx_gram_cross_vjp_workspace_bytes(ctypes.byref(big), 16, 1) > lib.mfx_gram_cross_workspace_bytes(ctypes.byref(big), 16)


def test_non_gram_operator_is_refused_like_the_forward():
    dense = _lib.Operator()
    dense.kind, dense.dtype, dense.n, dense.dense_a, dense.lda = _lib.OP_DENSE, _lib.MFX_F32, 4, 64, 4
    lib = _lib.get()
    assert lib.mfx_gram_cross_apply(ctypes.byref(dense), FAKE, 7, FAKE, 4, FAKE, 7, 2, FAKE, 1 << 30, None) == UNSUPPORTED
    assert _apply_t(dense) == UNSUPPORTED and "kernel-Gram" in _err()
    assert _vjp(dense, grads=_grads(dense_a=64)) == UNSUPPORTED and "kernel-Gram" in _err()


@pytest.mark.parametrize("kw", [dict(m=0), dict(ldu=6), dict(ldy=299), dict(p=0), dict(u=None)])
def test_transpose_refuses_bad_sizes_and_nulls(kw):
    assert _apply_t(_rbf(), **kw) == INVALID
    assert "mfx_gram_cross_apply_t" in _err()


@pytest.mark.parametrize("kw", [dict(m=0), dict(ldl=6), dict(ldr=299), dict(batch=0), dict(xnew=None)])
def test_vjp_refuses_bad_sizes_and_nulls(kw):
    assert _vjp(_rbf(), **kw) == INVALID
    assert "mfx_gram_cross_vjp" in _err()


def test_vjp_refuses_a_null_grads_struct():
    lib = _lib.get()
    desc = _rbf()
    assert lib.mfx_gram_cross_vjp(ctypes.byref(desc), FAKE, 7, FAKE, 7, FAKE, 300, 2, None, FAKE, FAKE, 1 << 30, None) == INVALID


@pytest.mark.parametrize("field", ["dense_a", "val"])
def test_vjp_refuses_fields_of_other_operators(field):
    assert _vjp(_rbf(), grads=_grads(**{field: 64, "outputscale": 64})) == INVALID
    assert "dense_a / val" in _err()


def test_row_blocks_are_unsupported():
    rows = _rbf(nrows=64)
    assert _apply_t(rows) == UNSUPPORTED and "row block" in _err()
    assert _vjp(rows) == UNSUPPORTED and "row block" in _err()


def test_too_wide_inputs_are_unsupported():
    wide = _rbf(d=1025)
    assert _apply_t(wide) == UNSUPPORTED and "d <= 1024" in _err()
    assert _vjp(wide) == UNSUPPORTED and "d <= 1024" in _err()


def test_null_operator_data_is_invalid():
    desc = _rbf()
    desc.x = None
    assert _apply_t(desc) == INVALID and "null" in _err()
    assert _vjp(desc) == INVALID and "null" in _err()


def test_short_workspace_is_refused():
    lib = _lib.get()
    desc = _rbf(n=4096, d=8)
    need_t = lib.mfx_gram_cross_workspace_bytes(ctypes.byref(desc), 7)
    need_v = lib.mfx_gram_cross_vjp_workspace_bytes(ctypes.byref(desc), 7, 2)
    assert _apply_t(desc, ldy=4096, ws_bytes=need_t - 512) == WORKSPACE and "workspace" in _err()
    assert _apply_t(desc, ldy=4096, ws=None) == WORKSPACE
    assert _vjp(desc, ldr=4096, ws_bytes=need_v - 512) == WORKSPACE and "workspace" in _err()
    assert _vjp(desc, ldr=4096, ws=None) == WORKSPACE
