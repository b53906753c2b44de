"""The guard-banded checker itself (tests/_guard.py), on host arenas: it
must accept a correct copy and name every kind of wrong one. No GPU."""
import numpy as np
import pytest

from _guard import GUARD, GuardedCopy, Region


def _host_case(src, dst):
    return GuardedCopy(11, src, dst, src_on_host=True, dst_on_host=True)


def _do_copy(case):
    case.dst_buf[case.dst.indices()] = case.src_buf[case.src.indices()]


def test_prefill_never_matches_and_correct_copy_passes():
    case = _host_case(Region(3, 7, 48, 64), Region(5, 7, 48, 80))
    assert not (case.dst_buf[case.dst.indices()]
                == case.src_buf[case.src.indices()]).any()
    with pytest.raises(AssertionError, match="row 0 col 0"):
        case.check("untouched")
    _do_copy(case)
    case.check("copied")


@pytest.mark.parametrize(
    "rel,where",
    [(-1, "guard"), (11 + 4 * 16 + 5, "guard"), (0, "head"), (10, "head"),
     (11, "bulk \\(16B element 0\\)"), (11 + 4 * 16, "tail")])
def test_flat_failure_is_located(rel, where):
    # offset 5: 11-byte head, 4 bulk elements, 5-byte tail
    n = 11 + 4 * 16 + 5
    case = _host_case(Region.flat(5, n), Region.flat(5, n))
    _do_copy(case)
    case.dst_buf[case.dst.start + rel] ^= 0x01
    with pytest.raises(AssertionError, match=f"message offset {rel} "
                                             f"\\({where}\\)"):
        case.check("flipped")


def test_gap_and_source_damage_are_reported():
    case = _host_case(Region.flat(0, 3 * 48), Region(0, 3, 48, 80))
    _do_copy(case)
    case.dst_buf[GUARD + 80 + 48] ^= 0x80  # first gap byte after row 1
    with pytest.raises(AssertionError, match="gap after row 1"):
        case.check("gap")
    case.dst_buf[GUARD + 80 + 48] ^= 0x80
    case.check("restored")
    case.src_buf[GUARD + 7] ^= 0x01
    with pytest.raises(AssertionError, match="source arena modified"):
        case.check("source")


def test_expected_is_independent_of_live_buffers():
    case = _host_case(Region.flat(1, 100), Region.flat(2, 100))
    before = case.expected.copy()
    case.dst_buf[:] = 0
    case.src_buf[:] = 0
    assert np.array_equal(case.expected, before)
