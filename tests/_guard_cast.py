"""Guard-banded arenas for bit-exact converting-receive tests.

A sibling of ``_guard_accum.GuardedAccum``: the message holds elements of
one float type, the destination elements of another, and the expectation is
``msg.to(dtype)`` or, when accumulating, ``(dst.float() + msg.float())
.to(dtype)``, from torch on the CPU and never from the code under test.

* source and initial destination are slices of larger arenas of seeded
  random BIT PATTERNS (subnormals, huge and tiny magnitudes all occur);
  every random NaN/Inf pattern is made finite;
* on top of that, edge values are planted at fixed positions at the start of
  the message, as far as the message is long enough: every value of
  ``EDGES_F32`` that the source type can hold exactly (so each pair gets
  the ones that matter to it). When accumulating, the destination holds +0
  under them, so the sum is the value and the one rounding is the one under
  test;
* at most 8 results are NaN, at fixed positions (``NAN_AT``): NaNs planted
  in the source and, when accumulating, one in the destination and one
  +inf + -inf. The helper checks on the CPU that the reference is NaN at
  exactly those positions; there the verdict is "is NaN", everywhere else
  it is bitwise;
* an element outside the planted ones whose expectation would equal its
  initial destination bits is changed (destination bits flipped, or both
  sides set to 1 when accumulating), so an unwritten element can never look
  written;
* after the run the WHOLE destination arena must equal the expectation --
  bands and everything outside the message unchanged -- and the source
  arena must be unchanged.
"""
from __future__ import annotations

import numpy as np
import torch

from _guard import GUARD, _stream
from _guard_accum import DTYPES, finite_words

FLOATS = ("float32", "float16", "bfloat16")
PAIRS = [(d, s) for d in FLOATS for s in FLOATS if d != s]  # (dst, src)

# fp32 bit patterns of the edge values.
EDGES_F32 = np.array([
    0x00000000, 0x80000000,              # +0, -0
    0x7F800000, 0xFF800000,              # +inf, -inf
    0x477FE000,                          # 65504, fp16 max
    0x477FF000,                          # 65520, a tie that rounds to inf
    0x33800000,                          # 2^-24, the smallest fp16 subnormal
    0x33000000,                          # 2^-25, a tie that rounds to 0
    0x33002000,                          # 2^-25 * (1 + 2^-10), rounds up
    0x3F808000,                          # 1 + 2^-8, a bf16 tie, to 1
    0x3F818000,                          # 1 + 3 * 2^-8, a bf16 tie, up
    0x00000001, 0x007FFFFF, 0x80000001,  # fp32 subnormals
    0x7F7FFFFF,                          # fp32 max: overflows bf16
    0x7F7F8000,                          # the smallest that does (a tie)
    0xC77FF000, 0xBF808000,              # negative ties
], dtype=np.uint32)
assert np.float32(65504) == EDGES_F32[4:5].view(np.float32)[0]
assert np.float32(65520) == EDGES_F32[5:6].view(np.float32)[0]
assert np.float32(2.0 ** -24) == EDGES_F32[6:7].view(np.float32)[0]
assert np.float32(2.0 ** -25) == EDGES_F32[7:8].view(np.float32)[0]
assert np.float32(2.0 ** -25 * (1 + 2.0 ** -10)) == \
    EDGES_F32[8:9].view(np.float32)[0]
assert np.float32(1 + 2.0 ** -8) == EDGES_F32[9:10].view(np.float32)[0]
assert np.float32(1 + 3 * 2.0 ** -8) == EDGES_F32[10:11].view(np.float32)[0]

_SIGNED = {np.uint32: np.int32, np.uint16: np.int16}
_TSIGNED = {4: torch.int32, 2: torch.int16}


def itemsize(dtype: str) -> int:
    return np.dtype(DTYPES[dtype][1]).itemsize


def _tensor(words: np.ndarray, dtype: str):
    td, wt, *_ = DTYPES[dtype]
    return torch.from_numpy(words.view(_SIGNED[wt]).copy()).view(td)


def _words(t, dtype: str) -> np.ndarray:
    wt = DTYPES[dtype][1]
    return t.contiguous().view(_TSIGNED[t.element_size()]).numpy().view(
        wt).copy()


def edge_words(src_dtype: str) -> np.ndarray:
    """The edge values the source type holds exactly, as its words."""
    f = torch.from_numpy(EDGES_F32.view(np.int32).copy()).view(torch.float32)
    s = f.to(DTYPES[src_dtype][0])
    exact = (s.float().view(torch.int32) == f.view(torch.int32)).numpy()
    return _words(s, src_dtype)[exact]


def nan_word(dtype: str):
    _, wt, exp, *_ = DTYPES[dtype]
    return wt(exp | 1)  # a signalling pattern: payloads are not compared


def reference(dst_words, src_words, dst_dtype, src_dtype, accumulate):
    """Words of the expectation, from torch on the CPU."""
    s = _tensor(src_words, src_dtype)
    td = DTYPES[dst_dtype][0]
    if accumulate:
        r = (_tensor(dst_words, dst_dtype).float() + s.float()).to(td)
    else:
        r = s.to(td)
    return _words(r, dst_dtype)


class GuardedCast:
    """One converting case of `n` elements. `src_off` / `dst_off` are BYTE
    offsets of the message past the leading guards; the destination buffer
    handed to the engine holds `dst_cap` elements (default n)."""

    def __init__(self, seed: int, dst_dtype: str, src_dtype: str, n: int, *,
                 accumulate: bool = False, src_off: int = 0, dst_off: int = 0,
                 dst_cap: int | None = None, src_on_host: bool = False):
        assert dst_dtype != src_dtype
        ss, ds = itemsize(src_dtype), itemsize(dst_dtype)
        assert src_off % ss == 0 and dst_off % ds == 0
        self.dst_dtype, self.src_dtype, self.n = dst_dtype, src_dtype, n
        self.ss, self.ds, self.accumulate = ss, ds, accumulate
        self.tdtype = DTYPES[dst_dtype][0]
        self.dst_cap = n if dst_cap is None else dst_cap
        assert self.dst_cap >= n
        self.nbytes = n * ss          # the message's length
        self.s0, self.d0 = GUARD + src_off, GUARD + dst_off
        swt, dwt = DTYPES[src_dtype][1], DTYPES[dst_dtype][1]
        self.src_host = _stream(2 * seed + 1, self.s0 + n * ss + GUARD)
        self.dst_host = _stream(2 * seed + 2,
                                self.d0 + self.dst_cap * ds + GUARD)
        sw = self.src_host[self.s0:self.s0 + n * ss].copy().view(swt)
        dw = self.dst_host[self.d0:self.d0 + n * ds].copy().view(dwt)
        finite_words(sw, src_dtype)
        finite_words(dw, dst_dtype)
        # Planted values: edges first, then the NaN makers.
        edges = edge_words(src_dtype)[:n]
        k = edges.size
        sw[:k] = edges
        if accumulate:
            dw[:k] = 0
        nan_at = []

        def plant(src_word, dst_word=None):
            nonlocal k
            if k >= n:
                return
            sw[k] = src_word
            if dst_word is not None:
                dw[k] = dst_word
            nan_at.append(k)
            k += 1

        for _ in range(4):
            plant(nan_word(src_dtype))
        if accumulate:
            _, _, sexp, _, sone = DTYPES[src_dtype]
            _, _, dexp, _, _ = DTYPES[dst_dtype]
            plant(sone, nan_word(dst_dtype))          # 1 + NaN
            plant(swt(sexp), dwt(dexp | (1 << (8 * ds - 1))))  # inf + -inf
        planted = k
        self.nan_at = np.array(nan_at, dtype=np.int64)
        assert self.nan_at.size <= 8
        # No unplanted element may end where it started.
        exp = reference(dw, sw, dst_dtype, src_dtype, accumulate)
        clash = exp == dw
        clash[:planted] = False
        if accumulate:
            sw[clash] = DTYPES[src_dtype][4]
            dw[clash] = DTYPES[dst_dtype][4]
        else:
            dw[clash] ^= dwt(1)
        exp = reference(dw, sw, dst_dtype, src_dtype, accumulate)
        assert not (exp == dw)[planted:].any()
        # The reference is NaN exactly where NaNs were planted.
        is_nan = torch.isnan(_tensor(exp, dst_dtype).float()).numpy()
        assert np.array_equal(np.flatnonzero(is_nan), self.nan_at), \
            "reference NaNs are not exactly the planted ones"
        self.src_host[self.s0:self.s0 + n * ss] = sw.view(np.uint8)
        self.dst_host[self.d0:self.d0 + n * ds] = dw.view(np.uint8)
        self.src_words, self.dst_words, self.exp_words = sw, dw, exp
        self.expected = self.dst_host.copy()
        self.expected[self.d0:self.d0 + n * ds] = exp.view(np.uint8)
        # Live buffers; the *_host references are never handed to the code
        # under test.
        self.src_buf = self._place(self.src_host, src_on_host)
        self.dst_buf = self._place(self.dst_host, False)
        torch.cuda.synchronize()

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
        return self.src_buf.data_ptr() + self.s0

    @property
    def dst_ptr(self) -> int:
        return self.dst_buf.data_ptr() + self.d0

    # -- views for the engine ----------------------------------------------
    @property
    def src_view(self):
        """The message as the sender's buffer (bytes; a sender is typeless)."""
        return self.src_buf[self.s0:self.s0 + self.nbytes]

    @property
    def dst_view(self):
        """The receive buffer, `dst_cap` elements of the destination type."""
        return self.dst_buf[self.d0:self.d0 + self.dst_cap * self.ds].view(
            self.tdtype)

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
                f"(message offset {first - self.s0})")

    def check_against(self, expected: np.ndarray, label: str = "",
                      nan_at=None) -> None:
        """Bitwise, except the elements `nan_at`, which must be NaN."""
        got = self._fetch(self.dst_buf).copy()
        expected = expected.copy()
        nan_at = self.nan_at if nan_at is None else nan_at
        wt = DTYPES[self.dst_dtype][1]
        exp_mask = DTYPES[self.dst_dtype][2]
        for e in nan_at:
            at = self.d0 + int(e) * self.ds
            word = got[at:at + self.ds].view(wt)[0]
            if not ((word & wt(exp_mask)) == wt(exp_mask)
                    and (word & wt(~exp_mask & ~(1 << (8 * self.ds - 1))
                                   & (2 ** (8 * self.ds) - 1)))):
                raise AssertionError(
                    f"{label}: element {int(e)} must be NaN, is "
                    f"0x{int(word):x}")
            got[at:at + self.ds] = expected[at:at + self.ds]
        if not np.array_equal(got, expected):
            bad = np.flatnonzero(got != expected)
            first = int(bad[0])
            rel = first - self.d0
            where = ("guard or outside the message"
                     if rel < 0 or rel >= self.n * self.ds
                     else f"element {rel // self.ds}")
            raise AssertionError(
                f"{label}: {bad.size} wrong destination byte(s); first at "
                f"message offset {rel} ({where}): got 0x{int(got[first]):02x}"
                f", expected 0x{int(expected[first]):02x} "
                f"[{self.src_dtype} -> {self.dst_dtype}, n={self.n}, "
                f"accumulate={self.accumulate}]")

    def check(self, label: str = "") -> None:
        self.check_against(self.expected, label)
        self.check_source(label)

    def check_untouched(self, label: str = "") -> None:
        self.check_against(self.dst_host, label + " (must be untouched)",
                           nan_at=())
        self.check_source(label)
