"""The accumulate tests' own reference (tests/_guard_accum.py), pinned on
the CPU against hand-worked bit patterns: if the reference were wrong, the
bit-exact GPU tests would be wrong with it."""
import numpy as np
import pytest

pytest.importorskip("torch")

from _guard_accum import DTYPES, finite_words, reference_sum  # noqa: E402


def _sum(dtype, d, s):
    wt = DTYPES[dtype][1]
    return [int(x) for x in reference_sum(np.array(d, dtype=wt),
                                          np.array(s, dtype=wt), dtype)]


def test_finite_words_touches_nan_and_inf_patterns_only():
    w = np.array([0x7C00, 0xFC01, 0x7BFF, 0x0001, 0x8000], dtype=np.uint16)
    assert list(finite_words(w, "float16")) == [
        0x3C00, 0xBC01, 0x7BFF, 0x0001, 0x8000]
    w = np.array([0x7F80, 0xFFFF, 0x7F7F], dtype=np.uint16)
    assert list(finite_words(w, "bfloat16")) == [0x3F80, 0xBFFF, 0x7F7F]
    w = np.array([0x7F800000, 0xFFC00000, 0x7F7FFFFF], dtype=np.uint32)
    assert list(finite_words(w, "float32")) == [
        0x3F800000, 0xBFC00000, 0x7F7FFFFF]
    w = np.array([0x7F800000, 0xFFFFFFFF], dtype=np.uint32)
    assert list(finite_words(w, "int32")) == [0x7F800000, 0xFFFFFFFF]


def test_reference_sum_float16():
    assert _sum("float16", [0x7BFF], [0x7BFF]) == [0x7C00]  # overflow: inf
    assert _sum("float16", [0x0001], [0x0001]) == [0x0002]  # subnormals kept
    assert _sum("float16", [0x0400], [0x8001]) == [0x03FF]  # lands subnormal
    # 1 + 2^-11 is a tie between 1 and 1 + 2^-10: to even, both ways.
    assert _sum("float16", [0x3C00], [0x1000]) == [0x3C00]
    assert _sum("float16", [0x3C01], [0x1000]) == [0x3C02]


def test_reference_sum_bfloat16():
    # 1 + 2^-8 is a tie between 1 and 1 + 2^-7: to even, both ways.
    assert _sum("bfloat16", [0x3F80], [0x3B80]) == [0x3F80]
    assert _sum("bfloat16", [0x3F81], [0x3B80]) == [0x3F82]
    assert _sum("bfloat16", [0x7F7F], [0x7F7F]) == [0x7F80]  # overflow: inf
    assert _sum("bfloat16", [0x0001], [0x0001]) == [0x0002]  # subnormals kept


def test_reference_sum_float32_and_int32():
    assert _sum("float32", [0x00000001], [0x00000001]) == [0x00000002]
    assert _sum("float32", [0x3F800000], [0x3F800000]) == [0x40000000]
    assert _sum("int32", [0x7FFFFFFF], [0x00000001]) == [0x80000000]  # wraps
    assert _sum("int32", [0xFFFFFFFF], [0x00000002]) == [0x00000001]
