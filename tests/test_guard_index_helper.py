"""tests/_guard_index.py itself, on host arenas: the numpy expectation, the
complemented destination bytes and what check() reports."""
import numpy as np
import pytest

from _guard_index import GUARD, GuardedIndex, Pool, dense
from _guard_nd import View


def _host_case(seed, src, dst):
    return GuardedIndex(seed, src, dst, src_on_host=True, dst_on_host=True)


def _copy(case):
    """The copy under test, done by hand: byte by byte in message order."""
    case.dst_buf[case.dst.indices()] = case.src_buf[case.src.indices()]


SRC = Pool(16, 9, 768, 784, (8, 0, 4, 4, 2, 7))
DST = Pool(32, 7, 1152, 1168, (6, 0, 3, 5))


def test_expectation_is_pool_indexing():
    case = _host_case(1, SRC, DST)
    src_pool = SRC.of(case.src_host)
    want = case.dst_host.copy()
    DST.of(want)[list(DST.index)] = \
        src_pool[list(SRC.index)].reshape(len(DST.index), DST.slice_bytes)
    assert np.array_equal(case.expected, want)
    assert case.msg.size == SRC.nbytes == DST.nbytes == 4608
    # No destination byte already holds what is to land on it.
    assert not np.any(case.dst_host[DST.indices()] == case.msg)
    with pytest.raises(AssertionError, match="wrong destination"):
        case.check("nothing copied")
    case.check_untouched()
    _copy(case)
    case.check("copied")
    with pytest.raises(AssertionError, match="was written"):
        case.check_untouched()


def test_check_names_the_stray_byte():
    case = _host_case(2, SRC, dense(0, SRC.nbytes))
    _copy(case)
    case.check()
    case.dst_buf[GUARD - 1] ^= 1
    with pytest.raises(AssertionError, match="guard"):
        case.check()
    case.dst_buf[GUARD - 1] ^= 1
    gap = _host_case(3, dense(0, DST.nbytes), DST)
    _copy(gap)
    gap.dst_buf[DST.start + 1 * DST.pitch] ^= 1  # slice 1 is not picked
    with pytest.raises(AssertionError, match="unpicked slice or gap"):
        gap.check()
    gap.dst_buf[DST.start + 1 * DST.pitch] ^= 1
    gap.src_buf[GUARD] ^= 1
    with pytest.raises(AssertionError, match="source arena modified"):
        gap.check()


def test_nd_side_and_empty_index():
    window = View(64, (4, 9, 32), (160, 4 * 160 + 32, 4), 4)  # 4608 B
    case = _host_case(4, SRC, window)
    _copy(case)
    case.check("pool -> N-D window")
    empty = _host_case(5, Pool(0, 5, 64, 80, ()), dense(0, 0))
    assert empty.msg.size == 0
    empty.check("empty")
    empty.check_untouched("empty")
