"""tests/_guarded_ws.py on host memory: the allocator that the GPU contract tests trust has to notice what it is there to notice."""

import threading

import pytest
import torch

from _guarded_ws import LEAD, GuardedWs, trail_bytes

CPU = torch.device("cpu")


def test_view_is_exactly_the_request_between_two_poisoned_bands():
    g = GuardedWs(0xFF)
    for need in (0, 1, 255, 256, 70000, (1 << 20) + 1, 3 << 20):
        ws = g.take(need, CPU)
        rec = g.interior(ws)
        assert ws.numel() == need and ws.dtype == torch.uint8
        assert ws.storage_offset() == LEAD and LEAD % 256 == 0
        trail = rec.full.numel() - LEAD - need
        assert trail == trail_bytes(need) and trail % 256 == 0 and trail >= max(1 << 20, need)
        assert bool((rec.full == 0xFF).all())
    g.verify()


def test_identical_requests_share_a_repoisoned_buffer_and_other_sizes_never_do():
    g = GuardedWs(0x00)
    a = g.take(1000, CPU)
    a.fill_(7)
    g.poison = 0xFF
    b = g.take(1000, CPU)
    assert b is a and bool((g.interior(b).full == 0xFF).all())
    c = g.take(999, CPU)
    assert c.data_ptr() != a.data_ptr() and g.interior(c) is not g.interior(a)
    g.verify()
    assert g.handed_out == 3


def test_a_busy_buffer_is_not_handed_out_again():
    busy = set()
    g = GuardedWs(0x00, busy=busy)
    outer = g.take(512, CPU)
    busy.add(id(outer))
    outer.fill_(3)  # the state of the call in progress
    inner = g.take(512, CPU)
    assert inner is not outer and bool((outer == 3).all())
    busy.discard(id(outer))
    assert g.take(512, CPU) is outer
    g.verify()


@pytest.mark.parametrize("offset,band", [(0, "trail"), (255, "trail"), ((1 << 20) - 1, "trail"), (-4096 - 1, "lead")])
def test_a_write_outside_the_request_is_reported_with_its_offsets(offset, band):
    need = 4096
    g = GuardedWs(0xFF)
    ws = g.take(need, CPU, label="the_entry_point")
    g.interior(ws).full[LEAD + need + offset] = 0
    with pytest.raises(AssertionError) as err:
        g.verify()
    msg = str(err.value)
    assert "the_entry_point" in msg and f"need {need} bytes" in msg and band in msg and f"{offset:+d} .. {offset:+d}" in msg
    g.interior(ws).full[LEAD + need + offset] = 0xFF
    g.verify()


def test_an_overrun_is_not_forgotten_when_the_buffer_is_reused():
    g = GuardedWs(0x00)
    ws = g.take(300, CPU)
    g.interior(ws).full[LEAD + 300] = 1  # one byte past the end
    assert g.take(300, CPU) is ws  # re-poisoned: the byte itself is gone
    with pytest.raises(AssertionError, match=r"offsets \+0 \.\. \+0"):
        g.verify()
    g.verify()  # reported once


def test_the_default_label_names_the_caller():
    g = GuardedWs(0x00)

    def some_wrapper():
        return g.take(64, CPU)

    assert "some_wrapper" in g.interior(some_wrapper()).label


def test_threads_get_their_buffers_without_losing_any():
    g = GuardedWs(0x00)
    seen = [None] * 8

    def body(i):
        seen[i] = [g.take(100 + i, CPU) for _ in range(50)][-1]

    threads = [threading.Thread(target=body, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert g.handed_out == 400 and len({t.data_ptr() for t in seen}) == 8
    g.verify()
