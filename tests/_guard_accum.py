"""Guard-banded arenas for bit-exact accumulate (reducing receive) tests.

A sibling of ``_guard.GuardedCopy``: the same arenas and bands, but the
expectation inside the message region is a sum, not the source bytes.

* source and initial destination are seeded random BIT PATTERNS from numpy
  on the CPU, so subnormals, both zeros, huge and tiny magnitudes all occur;
  every NaN/Inf pattern (exponent all ones) is made finite by clearing its
  top exponent bit. Finite inputs never sum to NaN, fp16 sums do overflow to
  inf and do land on subnormals: all of that is wanted and well defined;
* the expectation comes from torch on the CPU, never from the code under
  test: ``(d.float() + s.float()).to(dtype)`` for the float types, ``d + s``
  (wrapping) for int32;
* an element whose sum would equal its initial destination bits (a zero in
  the source, or one too small to matter) is replaced on both sides by 1,
  so an unwritten element can never look written;
* after the run the WHOLE destination arena must equal the expectation --
  bands and everything outside the message unchanged, the message region
  the reference sum -- and the source arena must be unchanged.

Comparisons are on raw bytes. Nothing here takes a tolerance.
"""
from __future__ import annotations

import numpy as np
import torch

from _guard import GUARD, Region, _stream

# name -> (torch dtype, numpy word type, exponent mask, top exponent bit,
#          bit pattern of 1)
DTYPES = {
    "float32": (torch.float32, np.uint32, 0x7F800000, 0x40000000, 0x3F800000),
    "float16": (torch.float16, np.uint16, 0x7C00, 0x4000, 0x3C00),
    "bfloat16": (torch.bfloat16, np.uint16, 0x7F80, 0x4000, 0x3F80),
    "int32": (torch.int32, np.uint32, 0, 0, 1),
}


def itemsize(dtype: str) -> int:
    return np.dtype(DTYPES[dtype][1]).itemsize


def finite_words(words: np.ndarray, dtype: str) -> np.ndarray:
    """Clear the top exponent bit of every NaN/Inf pattern."""
    _, wt, exp, top, _ = DTYPES[dtype]
    if exp:
        bad = (words & wt(exp)) == wt(exp)
        words[bad] &= wt(~top & (2 ** (8 * words.itemsize) - 1))
    return words


def reference_sum(dst_words: np.ndarray, src_words: np.ndarray,
                  dtype: str) -> np.ndarray:
    """Words of the reference sum, from torch on the CPU."""
    td, wt, *_ = DTYPES[dtype]
    signed = {np.uint32: np.int32, np.uint16: np.int16}[wt]
    d = torch.from_numpy(dst_words.view(signed).copy()).view(td)
    s = torch.from_numpy(src_words.view(signed).copy()).view(td)
    if td == torch.int32:
        r = d + s
    else:
        r = (d.float() + s.float()).to(td)
        assert not torch.isnan(r.float()).any(), "finite inputs gave NaN"
    return r.view({4: torch.int32, 2: torch.int16}[r.element_size()]
                  ).numpy().view(wt).copy()


class GuardedAccum:
    """One accumulate case. The message is `nbytes` at `src_off` /
    `dst_off` past the leading guards; the destination buffer handed to the
    engine may be longer than the message (`dst_cap` bytes)."""

    def __init__(self, seed: int, dtype: str, nbytes: int, *,
                 src_off: int = 0, dst_off: int = 0, dst_cap: int | None = None,
                 src_on_host: bool = False, small_ints: bool = False):
        es = itemsize(dtype)
        assert nbytes % es == 0 and src_off % es == 0 and dst_off % es == 0
        self.dtype, self.es, self.nbytes = dtype, es, nbytes
        self.tdtype, wt, _, _, one = DTYPES[dtype]
        self.src = Region.flat(src_off, nbytes)
        self.dst = Region.flat(dst_off, nbytes)
        self.dst_cap = nbytes if dst_cap is None else dst_cap
        assert self.dst_cap >= nbytes and self.dst_cap % es == 0
        self.src_host = _stream(2 * seed + 1, self.src.arena_bytes())
        self.dst_host = _stream(
            2 * seed + 2, GUARD + dst_off + self.dst_cap + GUARD)
        s0, d0 = self.src.start, self.dst.start
        sw = self.src_host[s0:s0 + nbytes].copy().view(wt)
        dw = self.dst_host[d0:d0 + nbytes].copy().view(wt)
        if small_ints:
            # Small integer values: sums are exact in every type, so the
            # result does not depend on the order contributions arrive in.
            rng = np.random.default_rng(seed)
            td = self.tdtype
            sw = self._words(torch.from_numpy(
                rng.integers(1, 8, sw.size)).to(td), wt)
            dw = self._words(torch.from_numpy(
                rng.integers(-8, 8, dw.size)).to(td), wt)
        finite_words(sw, dtype)
        finite_words(dw, dtype)
        exp = reference_sum(dw, sw, dtype)
        clash = exp == dw
        sw[clash] = one
        dw[clash] = one
        exp = reference_sum(dw, sw, dtype)
        assert not (exp == dw).any()
        self.src_host[s0:s0 + nbytes] = sw.view(np.uint8)
        self.dst_host[d0:d0 + nbytes] = dw.view(np.uint8)
        self.src_words, self.dst_words = sw, dw
        self.expected = self.dst_host.copy()
        self.expected[d0:d0 + nbytes] = exp.view(np.uint8)
        # Live buffers; the *_host references are never handed to the code
        # under test.
        self.src_buf = self._place(self.src_host, src_on_host)
        self.dst_buf = self._place(self.dst_host, False)
        torch.cuda.synchronize()

    @staticmethod
    def _words(t, wt):
        signed = {4: torch.int32, 2: torch.int16}[t.element_size()]
        return t.view(signed).numpy().view(wt).copy()

    @staticmethod
    def _place(ref: np.ndarray, on_host: bool):
        if on_host:
            return ref.copy()
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

    # -- views for the engine ----------------------------------------------
    @property
    def src_view(self):
        """The message as the sender's buffer (bytes; a sender is typeless)."""
        s0 = self.src.start
        return self.src_buf[s0:s0 + self.nbytes]

    @property
    def dst_view(self):
        """The receive buffer, `dst_cap` bytes, in the dtype under test."""
        d0 = self.dst.start
        return self.dst_buf[d0:d0 + self.dst_cap].view(self.tdtype)

    # -- verdicts ------------------------------------------------------------
    def _fetch(self, buf) -> np.ndarray:
        if hasattr(buf, "cpu"):
            torch.cuda.synchronize()
            return buf.cpu().numpy()
        return buf

    def check_source(self, label: str = "") -> None:
        src_now = self._fetch(self.src_buf)
        if not np.array_equal(src_now, self.src_host):
            first = int(np.flatnonzero(src_now != self.src_host)[0])
            raise AssertionError(
                f"{label}: source arena modified at arena offset {first} "
                f"(message offset {first - self.src.start})")

    def check_against(self, expected: np.ndarray, label: str = "") -> None:
        got = self._fetch(self.dst_buf)
        if not np.array_equal(got, expected):
            bad = np.flatnonzero(got != expected)
            first = int(bad[0])
            rel = first - self.dst.start
            where = ("guard or outside the message"
                     if rel < 0 or rel >= self.nbytes
                     else f"element {rel // self.es}")
            raise AssertionError(
                f"{label}: {bad.size} wrong destination byte(s); first at "
                f"message offset {rel} ({where}): got 0x{int(got[first]):02x}"
                f", expected 0x{int(expected[first]):02x} [{self.dtype}, "
                f"src {self.src}, dst {self.dst}]")

    def check(self, label: str = "") -> None:
        self.check_against(self.expected, label)
        self.check_source(label)

    def check_untouched(self, label: str = "") -> None:
        self.check_against(self.dst_host, label + " (must be untouched)")
        self.check_source(label)
