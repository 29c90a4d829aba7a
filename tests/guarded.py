"""Guarded arena for buffer-contract tests (test infrastructure, no GPU needed).

Every array a test hands to the library is carved from one poisoned ``uint8``
tensor with a band of poison on either side, so a store outside the array
(a missed tail mask, a phantom replication, a block edge) lands in a band and
is found by :meth:`Arena.check`, and a load outside an input reads poison:

* poison ``0xA5``: every typed value of a band is negative (int32 0xA5A5A5A5,
  int64 likewise, float64 about -1.2e-130), so ``arrive``, ``req`` and ``mips``
  taken from a band are refused by the library's own validation or change the
  result;
* poison ``0x5A``: an int64 is about 6.5e18 (past the engine's 2^61-tick
  range), an int32 about 1.5e9.

The other poison also shows whether an output depends on what its buffer held
before the call.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

# Bytes of poison on each side of every view.  The replay kernels store their
# outputs 64 publishes at a time: one chunk of int64 is 512 B, so a band takes a
# store that is up to eight chunks off.
GUARD = 4096
# Base alignment of a view (misalign=False).  misalign=True starts the view at
# 256 * k + itemsize: the element type's natural alignment and no more.
ALIGN = 256


@dataclass
class View:
    name: str
    offset: int    # first byte, from the start of the arena
    nbytes: int
    itemsize: int

    @property
    def end(self) -> int:
        return self.offset + self.nbytes


class Arena:
    """One ``uint8`` tensor filled with ``poison``; typed views are handed out
    with at least GUARD bytes of poison of their own before and after."""

    def __init__(self, device, poison: int, nbytes: int = 1 << 22):
        assert 0 <= poison <= 0xFF
        self.device = torch.device(device)
        self.poison = int(poison)
        self.buf = torch.full((nbytes,), self.poison, dtype=torch.uint8, device=self.device)
        self.inside = torch.zeros(nbytes, dtype=torch.bool, device=self.device)  # "inside a view"
        self.views: list[View] = []
        self._cursor = 0

    def alloc(self, shape, dtype, misalign: bool = False, name: str | None = None) -> torch.Tensor:
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        base = self.buf.data_ptr()
        off = self._cursor + GUARD
        off += -(base + off) % ALIGN
        if misalign:
            off += itemsize
        if off + nbytes + GUARD > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} B is too small for {name or shape}")
        v = View(name or f"view{len(self.views)}", off, nbytes, itemsize)
        self.views.append(v)
        self.inside[off:off + nbytes] = True
        self._cursor = off + nbytes + GUARD  # the next view's band starts behind this one's
        t = self.buf[off:off + nbytes].view(dtype).view(shape)
        assert t.is_contiguous() and t.data_ptr() == base + off
        return t

    def fill(self, view: torch.Tensor, array) -> torch.Tensor:
        """Copy host data into a view (same shape and dtype: nothing is converted silently)."""
        src = torch.from_numpy(np.ascontiguousarray(array))
        if src.dtype != view.dtype or tuple(src.shape) != tuple(view.shape):
            raise TypeError(f"fill: {src.dtype}{tuple(src.shape)} into {view.dtype}{tuple(view.shape)}")
        view.copy_(src)
        return view

    def put(self, array, misalign: bool = False, name: str | None = None) -> torch.Tensor:
        """alloc + fill for a host array."""
        a = np.array(array, copy=True, order="C")
        return self.fill(self.alloc(a.shape, torch.from_numpy(a).dtype, misalign, name), a)

    def damage(self) -> str | None:
        """None if every byte outside the views still holds the poison, else a
        description of the first damaged byte."""
        bad = (self.buf != self.poison) & ~self.inside
        if not bool(bad.any()):
            return None
        i = int(torch.nonzero(bad)[0])
        n_bad = int(bad.sum())
        best = None
        for v in self.views:
            if i < v.offset:
                d, edge = i - v.offset, "start"      # -1: the byte just before the view
            else:
                d, edge = i - v.end + 1, "end"       # +1: the byte just after the view
            if best is None or abs(d) < abs(best[1]):
                best = (v, d, edge)
        if best is None:
            return f"byte {i} damaged ({n_bad} in all), no view handed out"
        v, d, edge = best
        elems = -(-abs(d) // v.itemsize)
        side = "before its start" if d < 0 else "past its end"
        return (f"'{v.name}' overran {side} by {elems} element(s): first damaged byte at {d:+d} from the view's "
                f"{edge} (arena byte {i}, value 0x{int(self.buf[i]):02X}, poison 0x{self.poison:02X}, "
                f"{n_bad} damaged byte(s) in all)")

    def check(self) -> None:
        msg = self.damage()
        assert msg is None, msg
