"""Sparse far-offset arenas for byte-exact copy tests past 4 GiB.

The discipline of tests/_guard_nd.py and tests/_guard_index.py, for messages
whose few bytes lie gigabytes apart. The sides are described exactly as
there (``View``, ``Pool``, ``dense``); their ``indices()`` give the byte
offsets of the message in message order, small arrays however far apart the
offsets are.

* An arena is ONE allocation of PORCH + BODY bytes; the base handed to the
  code under test is ``arena + PORCH``, and every offset below is relative
  to that base (so the porch is the negative offsets). It is never copied
  to the host whole.
* The whole arena is filled with the constant byte P. Only the *windows*
  hold data: the maximal runs of touched offsets, widened by GUARD bytes on
  each side and merged where they meet. Their bytes come from two seeded
  numpy streams on the CPU and are uploaded.
* A destination byte that equals the byte due to land on it is
  complemented, and so is a source message byte equal to P: an unwritten
  byte can never look written, and no message byte hides in the constant.
* The porch is there for the wrong addresses a kernel with broken offset
  arithmetic would form for an offset ``o`` (measured from the pointer the
  kernel was given): ``o`` modulo the wrap modulus, ``o`` minus the
  modulus, and the low half of ``o`` sign-extended. For every touched
  ``o >= modulus / 2`` all three must lie inside the arena and outside
  every window, or the case is rejected at construction: such a kernel
  then fails a comparison and does not fault.
* The expectation is numpy only: the destination windows with the message
  assigned through ``indices()``. ``check()`` demands (a) every destination
  window equal to it, (b) every byte of both arenas outside the windows
  still P -- counted where the arena lives, on the device with torch
  comparisons in chunks of at most CHUNK bytes -- and (c) every source
  window unchanged.

The wrap modulus is a parameter (2**32 on the device). With a modulus of
2**16 and host arenas the whole helper runs on the CPU, where
tests/test_guard_far_helper.py proves that check() rejects each of the
three wrong-address models.

Exact equality only; nothing here takes a tolerance.
"""
from __future__ import annotations

import numpy as np

from _guard_index import GuardedIndex, Pool, dense  # noqa: F401
from _guard_nd import GUARD, GuardedNd, View, _stream  # noqa: F401

P = 0xA5
_P64 = int.from_bytes(bytes([P]) * 8, "little", signed=True)
MODULUS = 2 ** 32
CHUNK = 256 << 20
GIB = 1 << 30

ALIASES = ("offset modulo the modulus", "offset minus the modulus",
           "low half sign-extended")


def geometry(modulus: int) -> tuple:
    """(porch, body) bytes of an arena for a wrap modulus: half of it
    below the base, one and a sixteenth above."""
    return modulus // 2, modulus + modulus // 16


PORCH, BODY = geometry(MODULUS)   # 2 GiB, 4 GiB + 256 MiB
# What a module with two device arenas needs free: the arenas, one
# expectation of a little over 4 GiB, chunked temporaries, and headroom.
NEED_FREE = 32 * GIB


def windows_of(offsets: np.ndarray, guard: int = GUARD) -> np.ndarray:
    """The (k, 2) array of [start, end) windows: maximal runs of the
    touched offsets, each widened by `guard` bytes on both sides, merged
    where two of them touch or overlap."""
    o = np.unique(np.asarray(offsets, dtype=np.int64))
    if o.size == 0:
        return np.empty((0, 2), dtype=np.int64)
    # Runs [a, b) and [c, d) meet when c - guard <= b + guard.
    cut = np.flatnonzero(np.diff(o) - 1 > 2 * guard)
    first = np.concatenate(([o[0]], o[cut + 1]))
    last = np.concatenate((o[cut], [o[-1]]))
    return np.stack((first - guard, last + 1 + guard), axis=1)


def aliases_of(offsets: np.ndarray, start: int, modulus: int) -> np.ndarray:
    """(3, n) wrong addresses for `offsets`, whose kernel pointer is
    `start`: what the kernel gets when it forms the offset from its pointer
    modulo the modulus, minus the modulus, or with the low half
    sign-extended (rows in the order of ALIASES)."""
    rel = np.asarray(offsets, dtype=np.int64) - start
    low = rel % modulus
    sext = np.where(low >= modulus // 2, low - modulus, low)
    return start + np.stack((low, rel - modulus, sext))


def _inside(windows: np.ndarray, x: np.ndarray) -> np.ndarray:
    """Which of the offsets x lie inside one of the (sorted) windows."""
    if len(windows) == 0:
        return np.zeros(np.shape(x), dtype=bool)
    k = np.searchsorted(windows[:, 0], x, side="right") - 1
    return (k >= 0) & (x < windows[np.maximum(k, 0), 1])


class FarArena:
    """porch + body bytes in one allocation, on the device (a torch uint8
    tensor) or on the host (numpy). Offsets are relative to the base,
    ``allocation + porch``."""

    def __init__(self, modulus: int = MODULUS, on_host: bool = False):
        self.modulus = modulus
        self.porch, self.body = geometry(modulus)
        self.on_host = on_host
        n = self.porch + self.body
        if on_host:
            self.buf = np.empty(n, dtype=np.uint8)
        else:
            import torch

            self.buf = torch.empty(n, dtype=torch.uint8, device="cuda")
            assert self.buf.data_ptr() % 256 == 0, "allocator alignment"
        self.fill()

    # -- contents ----------------------------------------------------------
    def fill(self) -> None:
        if self.on_host:
            self.buf.fill(P)
        else:
            self.buf.fill_(P)

    def region(self, off: int, n: int):
        """The live bytes [off, off + n), as a view of the arena."""
        assert -self.porch <= off and off + n <= self.body, (off, n)
        return self.buf[self.porch + off:self.porch + off + n]

    def write(self, off: int, data: np.ndarray) -> None:
        if self.on_host:
            self.region(off, data.size)[:] = data
        else:
            import torch

            self.region(off, data.size).copy_(torch.from_numpy(data))

    def read(self, off: int, n: int) -> np.ndarray:
        r = self.region(off, n)
        if self.on_host:
            return r.copy()
        return r.cpu().numpy()

    @property
    def base(self):
        """The arena from its base on: what views for the engine start
        from (offset 0 is the first byte past the porch)."""
        return self.buf[self.porch:]

    @property
    def base_ptr(self) -> int:
        assert not self.on_host
        return self.buf.data_ptr() + self.porch

    # -- check (b): constant outside the windows ---------------------------
    def _gaps(self, windows: np.ndarray):
        at = -self.porch
        for a, b in np.asarray(windows, dtype=np.int64).reshape(-1, 2):
            if a > at:
                yield at, int(a)
            at = max(at, int(b))
        if at < self.body:
            yield at, self.body

    def _chunks(self, windows: np.ndarray):
        for a, b in self._gaps(windows):
            for c in range(a, b, CHUNK):
                yield c, min(b, c + CHUNK)

    def _clean_device(self, windows: np.ndarray) -> bool:
        """One pass on the device, one synchronisation: 8 bytes a compare
        wherever a gap is 8-byte aligned, so a 256 MiB chunk leaves a
        32 MiB temporary."""
        import torch

        bad = torch.zeros((), dtype=torch.int64, device=self.buf.device)
        for a, b in self._chunks(windows):
            a, b = a + self.porch, b + self.porch
            a8, b8 = min(b, -(-a // 8) * 8), max(a, b // 8 * 8)
            if a8 < b8:
                bad += (self.buf[a8:b8].view(torch.int64) != _P64).sum()
                edges = ((a, a8), (b8, b))
            else:
                edges = ((a, b),)
            for x, y in edges:
                if x < y:
                    bad += (self.buf[x:y] != P).sum()
        return int(bad.item()) == 0

    def stray(self, windows: np.ndarray):
        """None when every byte outside the windows equals P, else
        (count, first offset, its value)."""
        if not self.on_host and self._clean_device(windows):
            return None
        count, first, value = 0, None, None
        for a, b in self._chunks(windows):
            r = self.region(a, b - a) != P
            if self.on_host:
                n = int(np.count_nonzero(r))
            else:
                n = int(r.sum().item())
            if n and first is None:
                if self.on_host:
                    first = a + int(np.flatnonzero(r)[0])
                else:
                    first = a + int(r.nonzero()[0].item())
                value = int(self.read(first, 1)[0])
            count += n
        return (count, first, value) if count else None


class FarArenas:
    """The source and the destination arena of a module, allocated once;
    every case refills them with P."""

    def __init__(self, modulus: int = MODULUS, *, src_on_host: bool = False,
                 dst_on_host: bool = False):
        self.modulus = modulus
        self.src = FarArena(modulus, src_on_host)
        self.dst = FarArena(modulus, dst_on_host)


class _Packed:
    """The windows of one arena and their bytes, back to back."""

    def __init__(self, offsets: np.ndarray, seed: int):
        self.windows = windows_of(offsets)
        sizes = self.windows[:, 1] - self.windows[:, 0]
        self.cum = np.concatenate(([0], np.cumsum(sizes)))
        self.data = _stream(seed, int(self.cum[-1]))

    def pos(self, offsets: np.ndarray) -> np.ndarray:
        k = np.searchsorted(self.windows[:, 0], offsets, side="right") - 1
        return self.cum[k] + offsets - self.windows[k, 0]

    def pieces(self, data: np.ndarray):
        for (a, b), c in zip(self.windows, self.cum):
            yield int(a), data[int(c):int(c) + int(b - a)]


class GuardedFar:
    """One far copy case in the arenas of `arenas`. `src` and `dst` are
    each a View or a Pool, placed with their `start` relative to the
    arena's base."""

    def __init__(self, arenas: FarArenas, seed: int, src, dst):
        assert src.nbytes == dst.nbytes, (src, dst)
        self.arenas, self.src, self.dst = arenas, src, dst
        self.modulus = arenas.modulus
        self.si, self.di = src.indices(), dst.indices()
        assert np.unique(self.di).size == self.di.size, "destination repeats"
        self.spack = _Packed(self.si, 2 * seed + 1)
        self.dpack = _Packed(self.di, 2 * seed + 2)
        for side, offs, pack, arena in (
                (src, self.si, self.spack, arenas.src),
                (dst, self.di, self.dpack, arenas.dst)):
            w = pack.windows
            assert len(w) == 0 or (w[0, 0] >= -arena.porch and
                                   w[-1, 1] <= arena.body), \
                f"{side} does not fit the arena"
            self._assert_aliases(side, offs, w, arena)
        # Inputs.
        ps, pd = self.spack.pos(self.si), self.dpack.pos(self.di)
        hide = ps[self.spack.data[ps] == P]
        self.spack.data[hide] ^= 0xFF
        self.msg = self.spack.data[ps].copy()
        clash = pd[self.dpack.data[pd] == self.msg]
        self.dpack.data[clash] ^= 0xFF
        self.expected = self.dpack.data.copy()
        self.expected[pd] = self.msg
        self._upload()

    def _upload(self) -> None:
        for arena, pack in ((self.arenas.src, self.spack),
                            (self.arenas.dst, self.dpack)):
            arena.fill()
            for off, piece in pack.pieces(pack.data):
                arena.write(off, piece)
        self._sync()

    def _sync(self) -> None:
        a = self.arenas
        if not (a.src.on_host and a.dst.on_host):
            import torch

            torch.cuda.synchronize()

    def set_message(self, src_bytes: np.ndarray, dst_bytes: np.ndarray,
                    expected_bytes: np.ndarray) -> None:
        """Replace the message, the destination bytes under it and the
        bytes expected there (a reducing receive: a sum, not a copy). The
        caller keeps the discipline: nothing in `src_bytes` equals P,
        `expected_bytes` differs from `dst_bytes` in every element."""
        ps, pd = self.spack.pos(self.si), self.dpack.pos(self.di)
        assert not (src_bytes == P).any()
        self.spack.data[ps] = src_bytes
        self.msg = src_bytes.copy()
        self.dpack.data[pd] = dst_bytes
        self.expected = self.dpack.data.copy()
        self.expected[pd] = expected_bytes
        self._upload()

    def _assert_aliases(self, side, offs, windows, arena) -> None:
        m = self.modulus
        far = offs[offs - side.start >= m // 2]
        for name, al in zip(ALIASES, aliases_of(far, side.start, m)):
            keep = al != far   # below the modulus, modulo changes nothing
            o, al = far[keep], al[keep]
            out = (al < -arena.porch) | (al >= arena.body)
            assert not out.any(), \
                (f"alias ({name}) of offset {int(o[out][0])} at "
                 f"{int(al[out][0])} leaves the arena: {side}")
            hit = _inside(windows, al)
            assert not hit.any(), \
                (f"alias ({name}) of offset {int(o[hit][0])} at "
                 f"{int(al[hit][0])} falls in a window: {side}")

    # -- properties the tests assert ---------------------------------------
    @staticmethod
    def rel_offsets(side) -> np.ndarray:
        """Message byte offsets from the pointer the kernel is given."""
        return side.indices() - side.start

    def crosses(self, side) -> bool:
        """The side's offsets pass both half the modulus and the modulus."""
        rel = self.rel_offsets(side)
        return bool((rel >= self.modulus // 2).any() and
                    (rel >= self.modulus).any())

    # -- raw pointers for the kernel hooks ---------------------------------
    @property
    def src_ptr(self) -> int:
        return self.arenas.src.base_ptr + self.src.start

    @property
    def dst_ptr(self) -> int:
        return self.arenas.dst.base_ptr + self.dst.start

    def nd_args(self) -> tuple:
        """Positional arguments of _core._copy_nd_sync up to `itemsize`."""
        s, d = self.src, self.dst
        assert s.itemsize == d.itemsize
        return (self.dst_ptr, list(d.shape), list(d.strides), self.src_ptr,
                list(s.shape), list(s.strides), s.itemsize)

    @staticmethod
    def _index_side(ptr: int, side) -> tuple:
        if isinstance(side, Pool):
            return (ptr, list(side.index), side.slice_bytes, side.pitch)
        assert side == dense(side.off, side.nbytes), side
        return (ptr, None, 0, 0)

    def index_args(self) -> tuple:
        """Positional arguments of _core._copy_index_sync up to `bytes`."""
        return (*self._index_side(self.dst_ptr, self.dst),
                *self._index_side(self.src_ptr, self.src), self.src.nbytes)

    def strided_args(self) -> tuple:
        """Positional arguments of _core._copy_strided_sync up to
        `row_bytes`: both sides are (rows, row_bytes) byte views."""
        s, d = self.src, self.dst
        assert s.shape == d.shape and s.itemsize == d.itemsize == 1
        assert s.strides[1] == d.strides[1] == 1
        return (self.dst_ptr, d.strides[0], self.src_ptr, s.strides[0],
                s.shape[0], s.shape[1])

    # -- buffers and index= for the engine ---------------------------------
    @property
    def src_view(self):
        return GuardedIndex._view(self.arenas.src.base, self.src)

    @property
    def dst_view(self):
        return GuardedIndex._view(self.arenas.dst.base, self.dst)

    @property
    def src_kw(self) -> dict:
        return GuardedIndex._kw(self.src)

    @property
    def dst_kw(self) -> dict:
        return GuardedIndex._kw(self.dst)

    # -- verdict -----------------------------------------------------------
    def _name_alias(self, x: int) -> str:
        al = aliases_of(self.di, self.dst.start, self.modulus)
        names = []
        m = None
        for name, row in zip(ALIASES, al):
            hit = np.flatnonzero((row == x) & (row != self.di))
            if hit.size:
                names.append(name)
                m = int(hit[0])
        if not names:
            return "no alias of a message offset"
        return (f"the alias ({', '.join(names)}) of message byte {m} at "
                f"offset {int(self.di[m])}")

    def _window_faults(self, arena, pack, want, what) -> list:
        out = []
        for off, piece in pack.pieces(want):
            got = arena.read(off, piece.size)
            bad = np.flatnonzero(got != piece)
            if bad.size:
                at = off + int(bad[0])
                hit = np.flatnonzero(self.di == at) if what == "destination" \
                    else np.empty(0)
                where = f"message byte {int(hit[0])}" if hit.size \
                    else "guard or gap"
                out.append(
                    f"{bad.size} wrong {what} byte(s) in window [{off}, "
                    f"{off + piece.size}); first at arena offset {at} "
                    f"({where}): got 0x{int(got[bad[0]]):02x}, expected "
                    f"0x{int(piece[bad[0]]):02x}")
        return out

    def faults(self) -> list:
        self._sync()
        a = self.arenas
        out = self._window_faults(a.dst, self.dpack, self.expected,
                                  "destination")                      # (a)
        for arena, pack, what in ((a.dst, self.dpack, "destination"),
                                  (a.src, self.spack, "source")):     # (b)
            s = arena.stray(pack.windows)
            if s:
                count, first, value = s
                alias = f", {self._name_alias(first)}" \
                    if what == "destination" else ""
                out.append(
                    f"{count} byte(s) of the {what} arena outside its "
                    f"windows changed; first at arena offset {first}: "
                    f"0x{value:02x}{alias}")
        out += self._window_faults(a.src, self.spack, self.spack.data,
                                   "source")                          # (c)
        return out

    def check(self, label: str = "") -> None:
        out = self.faults()
        if out:
            raise AssertionError(
                f"{label}: " + "; ".join(out) +
                f" [src {self.src}, dst {self.dst}]")

    def check_untouched(self, label: str = "") -> None:
        """The destination windows still hold their initial bytes."""
        out = self._window_faults(self.arenas.dst, self.dpack,
                                  self.dpack.data, "destination")
        assert not out, f"{label}: destination was written: {out[0]}"
