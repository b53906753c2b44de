"""Direct, guard-banded, byte-exact tests of the N-D copy kernels in
csrc/kernels.hip (k_copy_nd<G>, k_copy_nd_tile<E>) and their dispatch,
through _core._copy_nd_sync on one device.

Each case runs through tests/_guard_nd.py: numpy is the reference, the
whole destination arena (guards and gaps included) is compared, the source
arena must stay unchanged. No tolerances.

block_cap=1 makes one 256-thread block walk the whole message (several
grid-stride passes), block_cap=2 two blocks.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from starway_amd import _core  # noqa: E402

from _guard_nd import GuardedNd, View  # noqa: E402

ITEMSIZES = [1, 2, 4, 8, 16]


def run(seed, src, dst, label, **kw):
    case = GuardedNd(seed, src, dst)
    _core._copy_nd_sync(*case.hook_args(), 0, **kw)
    case.check(f"{label} {kw}")


def plan(v: View, writable=False):
    return _core._plan_layout(list(v.shape), list(v.strides), v.itemsize,
                              writable)


# =============================================================================
# Generic path: k_copy_nd<G>
# =============================================================================


@pytest.mark.parametrize("itemsize", ITEMSIZES)
@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))))
def test_generic_permutations_to_contiguous_and_back(perm, itemsize):
    """The six permutations of a (5,7,9) tensor whose rows of 9 sit in a
    pitch of 10 (so the identity is strided too, with gaps). 315 elements:
    at itemsize 16 one block needs two passes, and dimension boundaries
    fall mid-stride."""
    es = itemsize
    strided = View(0, (5, 7, 9), (70 * es, 10 * es, es), es).permute(perm)
    flat = View.dense(0, strided.shape, es)
    seed = 100 * es + sum(p * 3 ** i for i, p in enumerate(perm))
    for cap in (1, 2):
        run(seed, strided, flat, f"pack {perm}", block_cap=cap,
            path="generic")
        run(seed + 50, flat, strided, f"unpack {perm}", block_cap=cap,
            path="generic")


@pytest.mark.parametrize("cap", [1, 2])
def test_generic_five_outer_dimensions(cap):
    """(2,3,2,3,2) over a 16-byte run, gaps at every level."""
    strided = View(0, (2, 3, 2, 3, 2, 16), (1136, 368, 176, 56, 24, 1), 1)
    assert len(plan(strided)[1]) == 5 and plan(strided)[0] == 16
    flat = View.dense(0, strided.shape, 1)
    run(300, strided, flat, "5-d pack", block_cap=cap, path="generic")
    run(301, flat, strided, "5-d unpack", block_cap=cap, path="generic")


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("itemsize", [2, 4])
def test_generic_different_shapes_on_the_two_sides(itemsize, cap):
    """A transposed (6,10) source into a (4,15) destination that is every
    second column of a (4,30) frame: only the total size agrees."""
    es = itemsize
    src = View(0, (6, 10), (es, 6 * es), es)
    dst = View(0, (4, 15), (30 * es, 2 * es), es)
    run(310 + es, src, dst, "reshape", block_cap=cap, path="generic")


@pytest.mark.parametrize("cap", [1, 2])
def test_generic_stride_zero_source(cap):
    """expand(): the source repeats one row / one column."""
    rows = View(0, (40, 24), (0, 4), 4)
    run(320, rows, View.dense(0, rows.shape, 4), "expand rows",
        block_cap=cap, path="generic")
    cols = View(0, (24, 40), (4, 0), 4)
    run(321, cols, View(16, (24, 40), (176, 4), 4), "expand cols",
        block_cap=cap, path="generic")


QUANTITIES = ["src_ptr", "dst_ptr", "src_stride", "dst_stride", "src_unit",
              "dst_unit"]


def granule_views(which, g):
    """Byte views whose every quantity is a multiple of 16 except `which`,
    whose lowest set bit is g (g=16: none). Both sides hold 16 x 96 B."""
    q = {"src_ptr": 0, "dst_ptr": 0, "src_stride": 64, "dst_stride": 64,
         "src_unit": 48, "dst_unit": 48}
    if which in ("src_ptr", "dst_ptr"):
        q[which] = 48 + g
    elif which in ("src_stride", "dst_stride"):
        q[which] = 64 + 48 + g
    elif which is not None:
        q[which] = 3 * g
    total = 16 * 96
    views = []
    for side in ("src", "dst"):
        unit = q[side + "_unit"]
        views.append(View(q[side + "_ptr"], (total // unit, unit),
                          (q[side + "_stride"], 1), 1))
    return views


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize(
    "which,g", [(None, 16)] + list(itertools.product(QUANTITIES,
                                                     [8, 4, 2, 1])))
def test_generic_every_granule(which, g, cap):
    every_granule(which, g, cap, wide_index=False)


def every_granule(which, g, cap, wide_index):
    src, dst = granule_views(which, g)
    case = GuardedNd(400 + 8 * QUANTITIES.index(which or "src_ptr") + g,
                     src, dst)
    assert _core._plan_granule(plan(src), plan(dst, True), case.src_ptr,
                               case.dst_ptr) == g
    _core._copy_nd_sync(*case.hook_args(), 0, block_cap=cap, path="generic",
                        wide_index=wide_index)
    case.check(f"granule {g} forced by {which}, wide_index={wide_index}")


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize(
    "which,g", [(None, 16)] + list(itertools.product(QUANTITIES,
                                                     [8, 4, 2, 1])))
def test_generic_every_granule_wide_index(which, g, cap):
    """k_copy_nd<G, uint64_t>, which production reaches only past 2**32 - 1
    granules (64 GiB at G = 16): the same cases, forced by the hook."""
    every_granule(which, g, cap, wide_index=True)


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("src_off,dst_off", [(1, 7), (7, 1), (1, 1)])
def test_generic_base_offsets(src_off, dst_off, cap):
    src = View(src_off, (7, 11, 3), (3, 21, 1), 1)   # permuted (11,7,3)
    dst = View(dst_off, (33, 7), (9, 1), 1)
    run(500 + 8 * src_off + dst_off, src, dst, "offsets", block_cap=cap,
        path="generic")


@pytest.mark.parametrize("path", ["auto", "generic"])
def test_zero_element_message_is_a_noop(path):
    src = View(0, (0, 5), (2, 20), 2)
    dst = View(0, (5, 0), (2, 10), 2)
    run(600, src, dst, "empty", block_cap=1, path=path)


# =============================================================================
# Tiled path: k_copy_nd_tile<E>
# =============================================================================


def transposed(E, batch, nA, nB, off=0):
    """Logical (batch, nA, nB) whose unit-stride dimension is A: rows along
    A hold three spare elements and batches one spare row plus 16 bytes, so
    a write into a gap or past an edge lands in checked bytes. batch == 1
    drops out: a plain 2-D transpose."""
    sB = (nA + 3) * E
    sbatch = (nB + 1) * sB + 16
    return View(off, (batch, nA, nB), (sbatch, E, sB), E)


def tile_extents(T):
    return [1, T - 1, T, T + 1, 2 * T + 3]


def tiled_shapes(E):
    """Each axis takes the five edge extents while the other stays at
    T + 1 (so both always cross a tile boundary)."""
    TA, TB = _core._ND_TILE[E]
    for nA in tile_extents(TA):
        yield nA, TB + 1
    for nB in tile_extents(TB):
        yield TA + 1, nB


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("E", ITEMSIZES)
def test_tiled_edges(E, batch):
    """Extents {1, T-1, T, T+1, 2T+3} on each tile axis, the transposed
    side as source and as destination, capped and uncapped grids.

    An extent of 1 is dropped by the normalisation, which leaves no
    transpose: the tiled kernel refuses that pair (ValueError) and the
    case is checked through path="auto" instead."""
    for k, (nA, nB) in enumerate(tiled_shapes(E)):
        s = transposed(E, batch, nA, nB)
        flat = View.dense(0, s.shape, E)
        seed = 1000 * E + 100 * batch + 2 * k
        if 1 in (nA, nB):
            for i, (src, dst) in enumerate([(s, flat), (flat, s)]):
                case = GuardedNd(seed + i, src, dst)
                with pytest.raises(ValueError):
                    _core._copy_nd_sync(*case.hook_args(), 0, path="tiled")
                case_auto = GuardedNd(seed + i, src, dst)
                _core._copy_nd_sync(*case_auto.hook_args(), 0, path="auto")
                case_auto.check(f"auto E={E} {nA}x{nB}")
            continue
        cap = 2 if k % 2 else 0  # alternate: two blocks loop over the tiles
        run(seed, s, flat, f"tiled pack E={E} b={batch} {nA}x{nB}",
            block_cap=cap, path="tiled")
        run(seed + 1, flat, s, f"tiled unpack E={E} b={batch} {nA}x{nB}",
            block_cap=cap, path="tiled")


def test_tiled_permute_with_two_batch_dimensions():
    """(2,3,A,B) -> A innermost in memory, batch dimensions on both sides
    of it in stride order."""
    E = 4
    TA, TB = _core._ND_TILE[E]
    nA, nB = TA + 5, TB + 2
    s = View(0, (2, 3, nA, nB),
             (nB * (nA + 1) * E, 2 * nB * (nA + 1) * E + 64, E, (nA + 1) * E),
             E)
    flat = View.dense(0, s.shape, E)
    run(2000, s, flat, "tiled 2 batch dims pack", block_cap=1, path="tiled")
    run(2001, flat, s, "tiled 2 batch dims unpack", path="tiled")


def test_tiled_refuses_ineligible_pairs():
    E = 4
    dense_rows = View(0, (6, 8, 4), (256, 16, 4), E)     # unit 16: no transpose
    both_strided = transposed(E, 1, 70, 70)
    misaligned = transposed(E, 1, 70, 70, off=2)          # base not E-aligned
    for src, dst in [
        (dense_rows, View.dense(0, dense_rows.shape, E)),
        (both_strided, View(0, (70, 70), (300, 4), E)),
        (misaligned, View.dense(0, misaligned.shape, E)),
    ]:
        case = GuardedNd(2100, src, dst)
        with pytest.raises(ValueError):
            _core._copy_nd_sync(*case.hook_args(), 0, path="tiled")
        # Nothing ran: the destination still holds its prefill.
        assert np.array_equal(case._fetch(case.dst_buf), case.dst_host)


def test_auto_matches_on_eligible_and_ineligible_pairs():
    E = 2
    TA, TB = _core._ND_TILE[E]
    eligible = transposed(E, 1, 2 * TA + 3, TB + 1)
    ineligible = View(0, (6, 8, 40), (2 * 40 * 9, 6 * 2 * 40 * 9, 2), E)
    for k, v in enumerate([eligible, ineligible]):
        flat = View.dense(0, v.shape, E)
        for path in ("auto", "generic"):
            run(2200 + k, v, flat, f"auto-vs-generic pack {k}", path=path)
            run(2210 + k, flat, v, f"auto-vs-generic unpack {k}", path=path)
