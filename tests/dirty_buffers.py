"""A replay allocator for tests: what does an entry point assume about memory it did not write?

Every Python wrapper takes its workspace and most of its outputs from ``torch.empty``.  In a test process such a tensor is very
often a fresh device allocation that reads as zeros, so a kernel that needs zeroed scratch (a counter, a ticket word, a "done" flag,
an accumulator) passes -- and one that needs ``~0`` (the empty slot of a hash table) passes wherever the block last held ``0xFF``.
``DirtyBuffers`` takes that luck away.  For the duration of a ``with`` block it replaces ``torch.empty``, ``torch.empty_like`` and
``Tensor.new_empty`` (through pytest's ``monkeypatch``; ``torch.zeros``, ``torch.full`` and friends are left alone) and hands out

    fill(byte)   tensors whose every byte is ``byte``: 0x00, or 0xFF (every int -1, every uint all ones, every float a NaN,
                 every bool True);
    replay()     to the k-th allocation of this run the very storage the k-th allocation of the run before had -- still holding
                 what that run left there -- provided shape, dtype and device are the same; otherwise a fresh 0xFF-filled tensor.
                 "The run before" is the previous ``with`` block of the same DirtyBuffers, whatever its mode.
    guarded()    tensors of zeros that are views into a larger buffer, with ``GUARD`` bytes of ``GUARD_BYTE`` in front of them and
                 behind them: does an entry point write outside the bytes it asked for?  The view starts at a multiple of 256 bytes
                 (the allocator's blocks start at multiples of 512 and GUARD is one), so the alignment rules of the C boundary hold
                 as they do for a tensor of its own.  ``damage()`` lists, after the run, every allocation with a changed guard byte.
                 A stray write lands in memory this allocator owns.

No aliasing: every tensor a run hands out stays referenced until the run after the next begins, so the allocator underneath cannot
give one block to two allocations of a run, and a replayed storage is handed out once per run (to the allocation with its index).
A test therefore clones what it wants to compare before it starts the next run.

There is no GPU code here: the fill is one ``fill_`` over the tensor's storage, enqueued on the current stream like the work of the
wrapper that asked for the tensor.
"""
import contextlib

import torch

__all__ = ["DirtyBuffers"]


GUARD = 4096
GUARD_BYTE = 0xA5


class DirtyBuffers:
    def __init__(self, monkeypatch):
        self._monkeypatch = monkeypatch
        self._real_empty = torch.empty
        self._real_empty_like = torch.empty_like
        self._real_new_empty = torch.Tensor.new_empty
        self._previous = []          # the tensors of the run before, in allocation order
        self._current = None         # the tensors of the run in progress
        self.replayed = 0            # of the run in progress / the last run: allocations that got an old storage
        self.fresh = 0               # ... and those that got a new one
        self._guards = []            # guarded(): (the whole buffer as uint8, where the view starts in it, the view's bytes) per allocation, in order

    # ---- the four modes -----------------------------------------------------------------------------------------------------
    def fill(self, byte):
        if not 0 <= int(byte) <= 0xFF:
            raise ValueError("fill byte outside 0..255")
        return self._run(lambda k, t: self._filled(t, int(byte)))

    def replay(self):
        return self._run(self._replayed)

    def guarded(self):
        self._guards = []
        return self._run(self._guarded)

    def damage(self):
        """of the last guarded run: (allocation index, its bytes, "front" / "back", changed guard bytes, offset of the first from the view's start)"""
        found = []
        for k, (whole, start, nbytes) in enumerate(self._guards):
            for side, first in (("front", start - GUARD), ("back", start + nbytes)):
                bad = torch.nonzero(whole[first:first + GUARD] != GUARD_BYTE).reshape(-1)
                if bad.numel():
                    found.append((k, nbytes, side, int(bad.numel()), first + int(bad[0]) - start))
        return found

    # ---- one run --------------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _run(self, finish):
        if self._current is not None:
            raise RuntimeError("DirtyBuffers runs do not nest")
        self._current, self.replayed, self.fresh = [], 0, 0

        def hand_out(t):
            if t.is_sparse or t.layout != torch.strided or t.device.type == "meta":
                return t
            t = finish(len(self._current), t)
            self._current.append(t)
            return t

        real_empty, real_empty_like, real_new_empty = self._real_empty, self._real_empty_like, self._real_new_empty

        def empty(*args, **kwargs):
            if kwargs.get("out") is not None:
                return real_empty(*args, **kwargs)
            return hand_out(real_empty(*args, **kwargs))

        def empty_like(*args, **kwargs):
            return hand_out(real_empty_like(*args, **kwargs))

        def new_empty(self_tensor, *args, **kwargs):
            return hand_out(real_new_empty(self_tensor, *args, **kwargs))

        try:
            with self._monkeypatch.context() as m:
                m.setattr(torch, "empty", empty)
                m.setattr(torch, "empty_like", empty_like)
                m.setattr(torch.Tensor, "new_empty", new_empty)
                yield self
        finally:
            self._previous, self._current = self._current, None

    def _bytes_of(self, t):
        """a uint8 tensor over the whole storage of t (no copy)"""
        storage = t.untyped_storage()
        return self._real_empty(0, dtype=torch.uint8, device=t.device).set_(storage, 0, (storage.nbytes(),), (1,))

    def _filled(self, t, byte):
        if t.untyped_storage().nbytes() > 0:
            self._bytes_of(t).fill_(byte)
        self.fresh += 1
        return t

    def _guarded(self, k, t):
        nbytes = t.untyped_storage().nbytes()
        whole = self._real_empty(GUARD + 256 + nbytes + GUARD, dtype=torch.uint8, device=t.device)
        start = GUARD + (-whole.data_ptr()) % 256          # (0 more on the device; a host block may start anywhere)
        assert t.storage_offset() == 0 and start % t.element_size() == 0, "the view would not start where a tensor of its own does"
        whole.fill_(GUARD_BYTE)
        whole[start:start + nbytes].zero_()
        view = self._real_empty(0, dtype=t.dtype, device=t.device).set_(whole.untyped_storage(), start // t.element_size(), t.shape, t.stride())
        if t.requires_grad:
            view.requires_grad_(True)
        self._guards.append((whole, start, nbytes))
        self.fresh += 1
        return view

    def _replayed(self, k, t):
        old = self._previous[k] if k < len(self._previous) else None
        if (old is None or old.shape != t.shape or old.dtype != t.dtype or old.device != t.device or old.stride() != t.stride()
                or old.storage_offset() != 0 or t.storage_offset() != 0 or old.untyped_storage().nbytes() == 0):
            return self._filled(t, 0xFF)
        again = self._real_empty(0, dtype=t.dtype, device=t.device).set_(old.untyped_storage(), 0, t.shape, t.stride())
        if t.requires_grad:
            again.requires_grad_(True)
        self.replayed += 1
        return again
