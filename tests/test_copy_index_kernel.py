"""The indexed copy kernel (k_copy_indexed) through _core._copy_index_sync:
every granule width, both directions, slices longer than a workgroup pass,
two indexed sides whose slice boundaries interleave, and the edges. Each
case runs with the default grid and with block_cap=1, which forces the
grid-stride loop. Byte-exact through tests/_guard_index.py.
"""
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from starway_amd import _core  # noqa: E402

from _guard_index import GuardedIndex, Pool, dense  # noqa: E402

CAPS = [0, 1]


def run(case: GuardedIndex, cap: int, label: str, wide_index: bool = False):
    _core._copy_index_sync(*case.hook_args(), 0, cap, wide_index=wide_index)
    case.check(f"{label} cap={cap} wide_index={wide_index}")


def both_ways(seed: int, pool: Pool, cap: int, label: str, flat_off: int = 0,
              wide_index: bool = False):
    """Gather pool[idx] into a dense run, and scatter a dense run into it.
    A source may repeat an entry; the scatter then takes the list without
    the repeat."""
    run(GuardedIndex(seed, pool, dense(flat_off, pool.nbytes)), cap,
        f"{label} gather", wide_index)
    uniq = tuple(dict.fromkeys(pool.index))
    spool = Pool(pool.off, pool.slices, pool.slice_bytes, pool.pitch, uniq)
    run(GuardedIndex(seed + 100, dense(flat_off, spool.nbytes), spool), cap,
        f"{label} scatter", wide_index)


# (label, pool, offset of the dense side): arenas are 256 B aligned, so the
# offsets alone decide the granule.
GRANULES = [
    ("16 B vector path", Pool(0, 11, 1040, 1072, (7, 0, 10, 3, 9)), 0),
    ("16 B, repeated source entry", Pool(0, 11, 1040, 1072, (7, 0, 10, 3, 3)),
     0),
    ("4 B granule", Pool(0, 11, 1044, 1052, (7, 0, 10, 3, 9)), 0),
    ("1 B granule", Pool(0, 11, 1041, 1043, (7, 0, 10, 3, 9)), 0),
    ("8 B granule, pool base shifted", Pool(8, 11, 1040, 1072,
                                            (7, 0, 10, 3, 9)), 0),
    ("8 B granule, dense base shifted", Pool(0, 11, 1040, 1072,
                                             (7, 0, 10, 3, 9)), 8),
    ("2 B granule", Pool(2, 11, 1042, 1046, (7, 0, 10, 3, 9)), 0),
    ("slice longer than a workgroup pass", Pool(0, 5, 20496, 20512,
                                                (4, 0, 2)), 0),
    ("slices of 8 KiB, no gap", Pool(0, 6, 8192, 8192, (5, 1, 0)), 0),
]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("label,pool,flat_off", GRANULES,
                         ids=[g[0] for g in GRANULES])
def test_gather_and_scatter(label, pool, flat_off, cap):
    both_ways(10 + GRANULES.index((label, pool, flat_off)), pool, cap, label,
              flat_off)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("label,pool,flat_off", GRANULES,
                         ids=[g[0] for g in GRANULES])
def test_gather_and_scatter_wide_index(label, pool, flat_off, cap):
    """k_copy_indexed<G, uint64_t>, which production reaches only past
    2**32 - 1 granules: the same table, forced by the hook."""
    both_ways(10 + GRANULES.index((label, pool, flat_off)), pool, cap, label,
              flat_off, wide_index=True)


def interleave(cap, wide_index):
    src = Pool(0, 9, 768, 784, (8, 0, 4, 5, 2, 7))
    dst = Pool(16, 7, 1152, 1168, (6, 0, 3, 5))
    assert src.nbytes == dst.nbytes == 4608
    run(GuardedIndex(30, src, dst), cap, "indexed -> indexed", wide_index)


@pytest.mark.parametrize("cap", CAPS)
def test_indexed_to_indexed_boundaries_interleave(cap):
    """Six 768 B source slices into four 1152 B destination slices: every
    destination slice is fed by two source slices and every second source
    slice is split over two destination slices."""
    interleave(cap, wide_index=False)


@pytest.mark.parametrize("cap", CAPS)
def test_indexed_to_indexed_boundaries_interleave_wide_index(cap):
    interleave(cap, wide_index=True)


@pytest.mark.parametrize("cap", CAPS)
def test_indexed_to_indexed_equal_slices(cap):
    src = Pool(0, 11, 1040, 1072, (7, 0, 10, 3, 3))
    dst = Pool(0, 8, 1040, 1040, (2, 7, 0, 5, 1))
    run(GuardedIndex(31, src, dst), cap, "indexed -> indexed, equal slices")


@pytest.mark.parametrize("cap", CAPS)
def test_edges(cap):
    one = Pool(0, 11, 1040, 1072, (6,))
    both_ways(40, one, cap, "count 1")
    # First and last slice of the pool: the guard bands on either side of
    # the arena catch an overshoot in either direction.
    ends = Pool(0, 11, 1040, 1072, (10, 0))
    both_ways(41, ends, cap, "first and last slice")


@pytest.mark.parametrize("cap", CAPS)
def test_count_zero_writes_nothing(cap):
    empty = Pool(0, 11, 1040, 1072, ())
    for case in (GuardedIndex(50, empty, dense(0, 0)),
                 GuardedIndex(51, dense(0, 0), empty)):
        _core._copy_index_sync(*case.hook_args(), 0, cap)
        case.check_untouched("count 0")
        case.check("count 0")
