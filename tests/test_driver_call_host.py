"""The host side of a libmfx driver call (operators.DriverCall, reduce_grads_, stash_params / rebuild_params) without a device and
without the library: stubs stand in for the ctypes entry points and a CPU uint8 tensor for the workspace."""

import types

import pytest
import torch

from matfree_extensions import _lib
from matfree_extensions.operators import CallbackOp, DriverCall, rebuild_params, reduce_grads_, stash_params

CPU = torch.device("cpu")


class _StubComm:
    def __init__(self, world):
        self.world, self.calls = world, 0

    def all_reduce_(self, t):
        self.calls += 1
        return t.mul_(2.0)


def test_reduce_grads_doubles_mixed_shapes_in_place_with_one_collective():
    comm = _StubComm(2)
    grads = (torch.arange(6.0).reshape(2, 3), torch.tensor(5.0), torch.tensor([1.0, -2.0]), torch.arange(8.0).reshape(2, 2, 2).mT)
    before = [g.clone() for g in grads]
    ptrs = [g.data_ptr() for g in grads]
    reduce_grads_(comm, grads)
    assert comm.calls == 1
    for g, b, ptr in zip(grads, before, ptrs):
        assert g.data_ptr() == ptr and g.shape == b.shape and torch.equal(g, 2.0 * b)


def test_reduce_grads_is_a_no_op_for_one_rank_or_no_gradients():
    one, two = _StubComm(1), _StubComm(2)
    g = torch.ones(3)
    reduce_grads_(one, (g,))
    reduce_grads_(two, ())
    assert one.calls == 0 and two.calls == 0 and torch.equal(g, torch.ones(3))


def test_stash_and_rebuild_round_trip_tensors_ints_and_none():
    a, b = torch.ones(2), torch.zeros((1, 3))
    params = (a, 3, None, b, "rbf", None, 0)
    ctx = types.SimpleNamespace()
    tensors = stash_params(ctx, params)
    assert len(tensors) == 2 and tensors[0] is a and tensors[1] is b
    assert not any(torch.is_tensor(q) for q in ctx.nontensor)
    out = rebuild_params(ctx, [t.clone() for t in tensors])  # (saved_tensors hands back other objects)
    assert len(out) == len(params)
    for q, w in zip(out, params):
        assert torch.equal(q, w) if torch.is_tensor(w) else (q is w if w is None else q == w)
    ctx = types.SimpleNamespace()
    assert stash_params(ctx, ()) == [] and rebuild_params(ctx, []) == ()


@pytest.fixture
def call(monkeypatch):
    """a DriverCall for a callback operator whose workspace is a CPU tensor; _lib.check records instead of asking the library"""
    ws = torch.zeros(64 + 256, dtype=torch.uint8)
    checked = []
    monkeypatch.setattr(_lib, "_take", lambda need, device: ws)
    monkeypatch.setattr(_lib, "check", checked.append)
    c = DriverCall(CallbackOp(lambda v: v), (), torch.float64, 4)
    queried = []
    assert c.take(lambda *a: queried.append(a) or 64, 4, 2, 1, device=CPU, visible=(torch.zeros(4, dtype=torch.float64), None)) is ws
    assert len(queried) == 1 and queried[0][1:] == (4, 2, 1)  # ONE size query: the descriptor, then the caller's dimensions
    c.checked = checked
    return c


def test_captured_exception_wins_over_the_status_as_the_same_object(call):
    exc = ZeroDivisionError("matvec failed on purpose")
    seen = []

    def entry(desc, a, b):
        seen.append((a, b, id(call.ws) in _lib._ws_busy))
        call.failure.append(exc)  # what the trampoline does when the Python matvec raises
        return 1

    with pytest.raises(ZeroDivisionError) as info:
        call.run(entry, 7, "x")
    assert info.value is exc
    assert seen == [(7, "x", True)]  # the arguments after the descriptor; the workspace is busy during the call
    assert call.checked == [] and not _lib._ws_busy


def test_status_is_checked_when_nothing_was_captured_and_busy_is_released_when_the_entry_raises(call):
    call.run(lambda desc: 0)
    call.run(lambda desc: -1)
    assert call.checked == [0, -1] and not _lib._ws_busy

    def entry(desc):
        assert id(call.ws) in _lib._ws_busy
        raise KeyError("inside the call")

    with pytest.raises(KeyError):
        call.run(entry)
    assert not _lib._ws_busy and call.checked == [0, -1]
