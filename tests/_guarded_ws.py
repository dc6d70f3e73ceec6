"""A guarded, poisoned stand-in for ``matfree_extensions._lib._take``: the workspace contract of include/mfx.h made checkable.

``_lib._take`` hands out ``need + 256`` bytes of a cached buffer that is usually far larger and still holds the results of an earlier
call.  A kernel that writes past the region it was given, a size query that under-reports, or a slot that is read without ever being
written are all invisible there.  ``GuardedWs.take`` has the same signature and gives the library exactly what it asked for:

    [ lead band | need bytes, handed to the library | trail band ]      every byte = ``poison`` when the buffer is handed out

  lead  = 65536 bytes; trail = max(1 MiB, need) rounded up to 256 -- an overrun by a whole mis-sized region still lands in the band;
  both are multiples of 256, so the view keeps the alignment the carvers assume.  ``numel()`` of the view is exactly ``need``.

A buffer is never reused for another ``need``; an identical (need, device, stream) gets the same buffer again, re-poisoned (the hipGraph
key of the Krylov drivers contains the workspace pointer, so repeated identical calls still reach capture and replay).  Before a
buffer is re-poisoned its bands are checked, so that a later call cannot wipe the traces of an earlier one.  ``verify()`` synchronises
and asserts that every band of every buffer handed out still holds the poison.  Thread-safe (tests/_local_world.py runs ranks as
threads) and re-entrant (a buffer that ``_lib.busy`` marks as in use is not handed out again: a second one is made).

Plain helper module: a test installs it with ``monkeypatch.setattr(_lib, "_take", guard.take)``.
"""

import os
import sys
import threading

import torch

LEAD = 65536
MIN_TRAIL = 1 << 20


def trail_bytes(need: int) -> int:
    return (max(MIN_TRAIL, int(need)) + 255) // 256 * 256


def _caller():
    """the first frame outside this module and _lib.py: which wrapper asked for the workspace"""
    skip = {os.path.abspath(__file__)}
    f = sys._getframe(1)
    while f is not None:
        path = os.path.abspath(f.f_code.co_filename)
        if path not in skip and os.path.basename(path) != "_lib.py":
            return f"{os.path.basename(path)}:{f.f_lineno} {getattr(f.f_code, 'co_qualname', f.f_code.co_name)}"
        f = f.f_back
    return "?"


class _Record:
    def __init__(self, full, view, need, poison, label):
        self.full, self.view, self.need, self.poison, self.label = full, view, need, poison, label


class GuardedWs:
    def __init__(self, poison: int = 0x00, busy=None):
        """busy: the set of id() of buffers in use (``_lib._ws_busy``), or None"""
        self.poison = int(poison) & 0xFF
        self._busy = busy if busy is not None else set()
        self._lock = threading.Lock()
        self._pool = {}  # (need, device, stream) -> [records]
        self._problems = []
        self.handed_out = 0

    # ---- the replacement of _lib._take -------------------------------------------------------------------------------------
    def take(self, need, device, label=None) -> torch.Tensor:
        need = int(need)
        if need < 0:
            raise ValueError(f"workspace request of {need} bytes")
        device = torch.device(device)
        stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
        key = (need, device.type, device.index, stream)
        label = label or _caller()
        with self._lock:
            self.handed_out += 1
            for rec in self._pool.setdefault(key, []):
                if id(rec.view) in self._busy:
                    continue
                self._problems += self._dirty(rec)  # before the traces of the last call are wiped
                rec.poison, rec.label = self.poison, label
                rec.full.fill_(rec.poison)
                return rec.view
            full = torch.full((LEAD + need + trail_bytes(need),), self.poison, dtype=torch.uint8, device=device)
            rec = _Record(full, full[LEAD : LEAD + need], need, self.poison, label)
            self._pool[key].append(rec)
            return rec.view

    # ---- checks ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _dirty(rec):
        if rec.full.is_cuda:
            torch.cuda.synchronize(rec.full.device)
        out = []
        end = LEAD + rec.need
        for name, lo, hi in (("lead", 0, LEAD), ("trail", end, rec.full.numel())):
            bad = (rec.full[lo:hi] != rec.poison).nonzero()
            if bad.numel():
                first, last = int(bad[0]) + lo - end, int(bad[-1]) + lo - end
                out.append(f"{rec.label}: need {rec.need} bytes, {name} band dirty: {bad.numel()} bytes, offsets {first:+d} .. {last:+d} "
                           f"from the end of the workspace (poison 0x{rec.poison:02X})")
        return out

    def verify(self):
        """every band of every buffer handed out so far still holds its poison"""
        with self._lock:
            problems, self._problems = self._problems, []
            for recs in self._pool.values():
                for rec in recs:
                    problems += self._dirty(rec)
        assert not problems, "workspace guard violated:\n  " + "\n  ".join(problems)

    def interior(self, view):
        """the record of a view ``take`` returned (tests that look at the workspace itself)"""
        with self._lock:
            for recs in self._pool.values():
                for rec in recs:
                    if rec.view is view:
                        return rec
        raise KeyError("not a buffer of this allocator")
