"""Guard-banded arenas for byte-exact N-D copy tests.

The discipline of tests/_guard.py, for arbitrary strided views:

* source and destination bytes come from two seeded numpy streams on the
  CPU and sit in arenas with a GUARD-byte band on each side;
* wherever a destination byte would equal the message byte that is to land
  on it, it is complemented -- an unwritten byte can never look written;
* the reference is numpy alone: ``np.lib.stride_tricks.as_strided`` over
  the host arena gives the message as ``.reshape(-1)`` of the source view
  (logical row-major order, what ``t.contiguous()`` holds) and the
  expectation by assignment through the destination view;
* after the copy the WHOLE destination arena must equal the expectation
  (a write into a gap between runs or past an edge fails) and the source
  arena must be unchanged.

Exact equality only; nothing here takes a tolerance.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from numpy.lib.stride_tricks import as_strided

GUARD = 256


@dataclass(frozen=True)
class View:
    """A strided view in an arena: `shape` in elements of `itemsize` bytes,
    `strides` in bytes, starting `off` bytes past the leading guard."""

    off: int
    shape: tuple
    strides: tuple
    itemsize: int

    @staticmethod
    def dense(off: int, shape, itemsize: int) -> "View":
        strides, run = [], itemsize
        for e in reversed(shape):
            strides.append(run)
            run *= e
        return View(off, tuple(shape), tuple(reversed(strides)), itemsize)

    def permute(self, perm) -> "View":
        return View(self.off, tuple(self.shape[p] for p in perm),
                    tuple(self.strides[p] for p in perm), self.itemsize)

    @property
    def nbytes(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64)) * self.itemsize

    @property
    def span(self) -> int:
        if self.nbytes == 0:
            return 0
        return sum((e - 1) * s for e, s in zip(self.shape, self.strides)) \
            + self.itemsize

    @property
    def start(self) -> int:
        return GUARD + self.off

    def arena_bytes(self) -> int:
        return GUARD + self.off + self.span + GUARD

    def of(self, arena: np.ndarray) -> np.ndarray:
        """This view over a host arena, as an array of opaque elements."""
        if self.nbytes == 0:
            return np.empty(self.shape, dtype=f"V{self.itemsize}")
        first = arena[self.start:self.start + self.itemsize]
        return as_strided(first.view(f"V{self.itemsize}"), self.shape,
                          self.strides)

    def indices(self) -> np.ndarray:
        """Arena offsets of the message bytes, in message order."""
        offs = np.zeros(1, dtype=np.int64)
        for e, s in zip(self.shape, self.strides):
            offs = (offs[:, None] + np.arange(e, dtype=np.int64) * s)
            offs = offs.reshape(-1)
        byte = np.arange(self.itemsize, dtype=np.int64)
        return (self.start + offs[:, None] + byte).reshape(-1)


def _stream(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


_TORCH_DTYPES = {1: "uint8", 2: "int16", 4: "int32", 8: "int64",
                 16: "complex128"}


class GuardedNd:
    """One N-D copy case: host reference arenas, device arenas,
    expectation."""

    def __init__(self, seed: int, src: View, dst: View, *,
                 src_on_host: bool = False, dst_on_host: bool = False):
        assert src.nbytes == dst.nbytes, (src, dst)
        self.src, self.dst = src, dst
        self.src_host = _stream(2 * seed + 1, src.arena_bytes())
        self.dst_host = _stream(2 * seed + 2, dst.arena_bytes())
        # The message: the source view in logical row-major order.
        self.msg = src.of(self.src_host).reshape(-1).copy()
        msg_bytes = self.msg.view(np.uint8)
        di = dst.indices()
        clash = self.dst_host[di] == msg_bytes
        self.dst_host[di[clash]] ^= 0xFF
        self.expected = self.dst_host.copy()
        if dst.nbytes:
            dst.of(self.expected)[...] = self.msg.reshape(dst.shape)
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

    # -- raw pointers for the kernel hook ----------------------------------
    @property
    def src_ptr(self) -> int:
        return self.src_buf.data_ptr() + self.src.start

    @property
    def dst_ptr(self) -> int:
        return self.dst_buf.data_ptr() + self.dst.start

    def hook_args(self) -> tuple:
        """Positional arguments of _core._copy_nd_sync up to `itemsize`."""
        s, d = self.src, self.dst
        assert s.itemsize == d.itemsize
        return (self.dst_ptr, list(d.shape), list(d.strides), self.src_ptr,
                list(s.shape), list(s.strides), s.itemsize)

    # -- views for the engine ----------------------------------------------
    @staticmethod
    def _view(buf, v: View):
        if not hasattr(buf, "as_strided"):
            # Host endpoints are contiguous.
            assert v == View.dense(v.off, v.shape, v.itemsize), v
            return buf[v.start:v.start + v.nbytes]
        import torch

        es = v.itemsize
        assert v.start % es == 0 and all(s % es == 0 for s in v.strides), v
        n = (buf.numel() - v.start) // es * es
        flat = buf[v.start:v.start + n].view(getattr(torch, _TORCH_DTYPES[es]))
        # No storage offset argument: it is absolute, and `flat` carries it.
        view = flat.as_strided(v.shape, [s // es for s in v.strides])
        assert v.nbytes == 0 or view.data_ptr() == buf.data_ptr() + v.start
        return view

    @property
    def src_view(self):
        return self._view(self.src_buf, self.src)

    @property
    def dst_view(self):
        return self._view(self.dst_buf, self.dst)

    # -- verdict -----------------------------------------------------------
    def _fetch(self, buf) -> np.ndarray:
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
            return "gap between runs"
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
