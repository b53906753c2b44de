"""Host tests of tests/_guard_nd.py itself: a copy emulated in numpy from
the planned layouts passes, and each kind of wrong copy is caught."""
import numpy as np
import pytest

from starway_amd import _core

from _guard_nd import GUARD, GuardedNd, View
from test_layout_plan import plan_offsets


def emulate(case: GuardedNd) -> None:
    """What the kernels do: message byte m goes from the source plan's
    m-th offset to the destination plan's."""
    s, d = case.src, case.dst
    so = plan_offsets(*_core._plan_layout(list(s.shape), list(s.strides),
                                          s.itemsize))
    do = plan_offsets(*_core._plan_layout(list(d.shape), list(d.strides),
                                          d.itemsize, True))
    case.dst_buf[d.start + do] = case.src_buf[s.start + so]


CASES = [
    (View(0, (6, 10), (2, 12), 2), View(0, (4, 15), (60, 4), 2)),
    (View(3, (7, 9, 5), (16, 112, 1600), 16), View.dense(5, (7, 9, 5), 16)),
    (View.dense(0, (3, 4, 5), 4), View(8, (3, 4, 5), (4, 12, 52), 4)),
    (View(0, (5, 8), (0, 1), 1), View(1, (8, 5), (1, 9), 1)),
]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_emulated_copy_passes(k):
    src, dst = CASES[k]
    case = GuardedNd(k, src, dst, src_on_host=True, dst_on_host=True)
    assert not np.array_equal(case.dst_buf, case.expected)
    emulate(case)
    case.check("emulated")


def test_wrong_copies_are_caught():
    src, dst = CASES[0]

    def fresh():
        c = GuardedNd(9, src, dst, src_on_host=True, dst_on_host=True)
        emulate(c)
        return c

    c = fresh()
    c.dst_buf[GUARD - 1] ^= 1          # one byte before the view
    with pytest.raises(AssertionError, match="guard"):
        c.check()
    c = fresh()
    c.dst_buf[dst.start + 2] ^= 1      # between two elements of a row
    with pytest.raises(AssertionError, match="gap"):
        c.check()
    c = fresh()
    c.dst_buf[dst.start + 4] ^= 1      # element (0, 1)
    with pytest.raises(AssertionError, match="message byte 2"):
        c.check()
    c = fresh()
    c.src_buf[src.start] ^= 1
    with pytest.raises(AssertionError, match="source arena modified"):
        c.check()
    # An untouched destination never passes: no byte already matches.
    c = GuardedNd(9, src, dst, src_on_host=True, dst_on_host=True)
    di = dst.indices()
    assert not (c.dst_buf[di] == c.expected[di]).any()
