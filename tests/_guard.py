"""Guard-banded arenas for byte-exact copy tests.

A copy's reference is its input, so every case here is built the same way:

* the source bytes come from a seeded numpy generator on the CPU and sit in
  a device arena with a GUARD-byte band on each side;
* the destination arena (bands and inter-row gaps included) is filled from
  a different seeded stream, and wherever a destination byte would equal
  the source byte that is to land on it, it is complemented -- an unwritten
  message byte can never look written;
* the expectation is computed in numpy on the host: the destination arena
  with the message bytes (or rows) replaced;
* after the copy the WHOLE destination arena must equal the expectation
  (so a write one element past the message, or into a gap between rows,
  fails) and the source arena must be unchanged.

Exact equality only; nothing here takes a tolerance.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

GUARD = 256


@dataclass(frozen=True)
class Region:
    """A message laid out in an arena: `rows` dense runs of `row_bytes`,
    `stride` bytes apart, starting `off` bytes past the leading guard.
    A contiguous message is one row."""

    off: int
    rows: int
    row_bytes: int
    stride: int

    @staticmethod
    def flat(off: int, nbytes: int) -> "Region":
        return Region(off, 1, nbytes, nbytes)

    @property
    def nbytes(self) -> int:
        return self.rows * self.row_bytes

    @property
    def span(self) -> int:
        if self.rows == 0 or self.row_bytes == 0:
            return 0
        return (self.rows - 1) * self.stride + self.row_bytes

    @property
    def start(self) -> int:
        return GUARD + self.off

    def indices(self) -> np.ndarray:
        """Arena offsets of the message bytes, in message order."""
        r = np.arange(self.rows, dtype=np.int64)[:, None] * self.stride
        c = np.arange(self.row_bytes, dtype=np.int64)[None, :]
        return (self.start + r + c).reshape(-1)

    def arena_bytes(self) -> int:
        return GUARD + self.off + self.span + GUARD


def _stream(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


class GuardedCopy:
    """One copy case: host reference arenas, device arenas, expectation."""

    def __init__(self, seed: int, src: Region, dst: Region, *,
                 src_on_host: bool = False, dst_on_host: bool = False):
        assert src.nbytes == dst.nbytes, (src, dst)
        self.src, self.dst = src, dst
        self.src_host = _stream(2 * seed + 1, src.arena_bytes())
        self.dst_host = _stream(2 * seed + 2, dst.arena_bytes())
        si, di = src.indices(), dst.indices()
        msg = self.src_host[si]
        clash = self.dst_host[di] == msg
        self.dst_host[di[clash]] ^= 0xFF
        self.expected = self.dst_host.copy()
        self.expected[di] = msg
        # Live buffers: device tensors (or host arrays for host endpoints).
        # The *_host reference copies above are never handed to the code
        # under test.
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

    # -- raw pointers for the kernel hooks ---------------------------------
    @property
    def src_ptr(self) -> int:
        return self.src_buf.data_ptr() + self.src.start

    @property
    def dst_ptr(self) -> int:
        return self.dst_buf.data_ptr() + self.dst.start

    # -- views for the engine ----------------------------------------------
    def _view(self, buf, reg: Region):
        if reg.rows == 1:
            return buf[reg.start:reg.start + reg.row_bytes]
        if hasattr(buf, "as_strided"):
            return buf.as_strided((reg.rows, reg.row_bytes), (reg.stride, 1),
                                  reg.start)
        raise ValueError("host endpoints are contiguous")

    @property
    def src_view(self):
        return self._view(self.src_buf, self.src)

    @property
    def dst_view(self):
        return self._view(self.dst_buf, self.dst)

    # -- verdict -------------------------------------------------------------
    def _where(self, arena_off: int) -> str:
        """Name the part of the destination an arena offset lies in."""
        d = self.dst
        rel = arena_off - d.start
        if rel < 0 or rel >= d.span:
            return "guard"
        row, col = divmod(rel, d.stride) if d.rows > 1 else (0, rel)
        if col >= d.row_bytes:
            return f"gap after row {row}"
        if d.rows > 1:
            return f"row {row} col {col}"
        # Contiguous: head / bulk / tail of the co-aligned dispatch.
        head = min((16 - d.off % 16) % 16, d.row_bytes)
        bulk_end = head + (d.row_bytes - head) // 16 * 16
        if rel < head:
            return "head"
        if rel < bulk_end:
            return f"bulk (16B element {(rel - head) // 16})"
        return "tail"

    def _fetch(self, buf) -> np.ndarray:
        if hasattr(buf, "cpu"):
            import torch

            torch.cuda.synchronize()
            return buf.cpu().numpy()
        return buf

    def check(self, label: str = "") -> None:
        got = self._fetch(self.dst_buf)
        if not np.array_equal(got, self.expected):
            bad = np.flatnonzero(got != self.expected)
            first = int(bad[0])
            raise AssertionError(
                f"{label}: {bad.size} wrong destination byte(s); first at "
                f"message offset {first - self.dst.start} "
                f"({self._where(first)}): got 0x{int(got[first]):02x}, "
                f"expected 0x{int(self.expected[first]):02x} "
                f"[src {self.src}, dst {self.dst}]")
        src_now = self._fetch(self.src_buf)
        if not np.array_equal(src_now, self.src_host):
            first = int(np.flatnonzero(src_now != self.src_host)[0])
            raise AssertionError(
                f"{label}: source arena modified at arena offset {first} "
                f"(message offset {first - self.src.start})")
