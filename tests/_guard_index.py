"""Guard-banded arenas for byte-exact indexed-copy tests (pool[idx]).

The discipline of tests/_guard_nd.py, for slices of a pool picked by an
index list:

* source and destination bytes come from two seeded numpy streams on the
  CPU and sit in arenas with a GUARD-byte band on each side;
* wherever a destination byte would equal the message byte that is to land
  on it, it is complemented -- an unwritten byte can never look written;
* the reference is numpy alone: a pool is a 2-D ``as_strided`` view
  (slices, slice_bytes) over the host arena, the message is
  ``src_pool[src_idx].reshape(-1)`` and the expectation is
  ``expected_pool[dst_idx] = message.reshape(len(dst_idx), slice_bytes)``;
* after the copy the WHOLE destination arena must equal the expectation (a
  write into an unpicked slice, into the gap between two slices or past an
  edge fails) and the source arena must be unchanged.

A side may also be a ``_guard_nd.View`` (a contiguous run, rows or an N-D
window), for the routes where an indexed buffer meets one.

Exact equality only; nothing here takes a tolerance.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from numpy.lib.stride_tricks import as_strided

from _guard_nd import GUARD, View, _stream


@dataclass(frozen=True)
class Pool:
    """`slices` runs of `slice_bytes` bytes, `pitch` bytes apart, starting
    `off` bytes past the leading guard; the message is the slices `index`
    names, in that order."""

    off: int
    slices: int
    slice_bytes: int
    pitch: int
    index: tuple

    @property
    def nbytes(self) -> int:
        return len(self.index) * self.slice_bytes

    @property
    def span(self) -> int:
        return (self.slices - 1) * self.pitch + self.slice_bytes

    @property
    def start(self) -> int:
        return GUARD + self.off

    def arena_bytes(self) -> int:
        return GUARD + self.off + self.span + GUARD

    def of(self, arena: np.ndarray) -> np.ndarray:
        """The whole pool over a host arena: (slices, slice_bytes) bytes."""
        first = arena[self.start:self.start + 1]
        return as_strided(first, (self.slices, self.slice_bytes),
                          (self.pitch, 1))

    def indices(self) -> np.ndarray:
        """Arena offsets of the message bytes, in message order."""
        rows = np.asarray(self.index, dtype=np.int64).reshape(-1, 1)
        cols = np.arange(self.slice_bytes, dtype=np.int64)
        return (self.start + rows * self.pitch + cols).reshape(-1)


def dense(off: int, nbytes: int) -> View:
    """One contiguous run of bytes."""
    return View.dense(off, (nbytes,), 1)


def _message(side, arena: np.ndarray) -> np.ndarray:
    if isinstance(side, Pool):
        return side.of(arena)[list(side.index)].reshape(-1)
    return side.of(arena).reshape(-1).copy().view(np.uint8)


def _assign(side, arena: np.ndarray, msg: np.ndarray) -> None:
    if side.nbytes == 0:
        return
    if isinstance(side, Pool):
        side.of(arena)[list(side.index)] = msg.reshape(len(side.index),
                                                       side.slice_bytes)
    else:
        side.of(arena)[...] = msg.view(f"V{side.itemsize}").reshape(side.shape)


class GuardedIndex:
    """One indexed copy case: host reference arenas, device arenas,
    expectation. `src` and `dst` are each a Pool or a View."""

    def __init__(self, seed: int, src, dst, *, src_on_host: bool = False,
                 dst_on_host: bool = False):
        assert src.nbytes == dst.nbytes, (src, dst)
        self.src, self.dst = src, dst
        self.src_host = _stream(2 * seed + 1, src.arena_bytes())
        self.dst_host = _stream(2 * seed + 2, dst.arena_bytes())
        self.msg = _message(src, self.src_host)
        di = dst.indices()
        clash = self.dst_host[di] == self.msg
        self.dst_host[di[clash]] ^= 0xFF
        self.expected = self.dst_host.copy()
        _assign(dst, self.expected, self.msg)
        self.src_buf = self._place(self.src_host, src_on_host)
        self.dst_buf = self._place(self.dst_host, dst_on_host)
        if not (src_on_host and dst_on_host):
            import torch

            torch.cuda.synchronize()

    @staticmethod
    def _place(ref: np.ndarray, on_host: bool):
        if on_host:
            return ref.copy()
        import torch

        buf = torch.from_numpy(ref.copy()).cuda()
        assert buf.data_ptr() % 256 == 0, "allocator alignment"
        return buf

    # -- the kernel hook ---------------------------------------------------
    @staticmethod
    def _side_args(buf, side) -> tuple:
        ptr = buf.data_ptr() + side.start
        if isinstance(side, Pool):
            return (ptr, list(side.index), side.slice_bytes, side.pitch)
        assert side == dense(side.off, side.nbytes), side
        return (ptr, None, 0, 0)

    def hook_args(self) -> tuple:
        """Positional arguments of _core._copy_index_sync up to `bytes`."""
        return (*self._side_args(self.dst_buf, self.dst),
                *self._side_args(self.src_buf, self.src), self.src.nbytes)

    # -- buffers and index= for the engine ---------------------------------
    @staticmethod
    def _view(buf, side):
        if not isinstance(side, Pool):
            from _guard_nd import GuardedNd

            return GuardedNd._view(buf, side)
        view = buf[side.start:].as_strided((side.slices, side.slice_bytes),
                                           (side.pitch, 1))
        assert view.data_ptr() == buf.data_ptr() + side.start
        return view

    @property
    def src_view(self):
        return self._view(self.src_buf, self.src)

    @property
    def dst_view(self):
        return self._view(self.dst_buf, self.dst)

    @staticmethod
    def _kw(side) -> dict:
        return {"index": list(side.index)} if isinstance(side, Pool) else {}

    @property
    def src_kw(self) -> dict:
        return self._kw(self.src)

    @property
    def dst_kw(self) -> dict:
        return self._kw(self.dst)

    # -- verdict -----------------------------------------------------------
    @staticmethod
    def _fetch(buf) -> np.ndarray:
        if hasattr(buf, "cpu"):
            import torch

            torch.cuda.synchronize()
            return buf.cpu().numpy()
        return buf

    def _where(self, arena_off: int) -> str:
        d = self.dst
        if arena_off < d.start or arena_off >= d.start + d.span:
            return "guard"
        hit = np.flatnonzero(d.indices() == arena_off)
        if hit.size == 0:
            return "unpicked slice or gap"
        return f"message byte {int(hit[0])}"

    def check(self, label: str = "") -> None:
        got = self._fetch(self.dst_buf)
        if not np.array_equal(got, self.expected):
            bad = np.flatnonzero(got != self.expected)
            first = int(bad[0])
            raise AssertionError(
                f"{label}: {bad.size} wrong destination byte(s); first at "
                f"arena offset {first} ({self._where(first)}): got "
                f"0x{int(got[first]):02x}, expected "
                f"0x{int(self.expected[first]):02x} "
                f"[src {self.src}, dst {self.dst}]")
        src_now = self._fetch(self.src_buf)
        if not np.array_equal(src_now, self.src_host):
            first = int(np.flatnonzero(src_now != self.src_host)[0])
            raise AssertionError(
                f"{label}: source arena modified at arena offset {first}")

    def check_untouched(self, label: str = "") -> None:
        """The destination arena still holds its initial bytes."""
        got = self._fetch(self.dst_buf)
        assert np.array_equal(got, self.dst_host), \
            f"{label}: destination arena was written"
