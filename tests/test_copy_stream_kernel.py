"""Guard-banded, byte-exact tests of the tile-contiguous streaming copy
(csrc/copy_stream.hpp) and of its route in launch_copy_tuned.

Every case runs through tests/_guard.py like tests/test_copy_kernels.py:
seeded CPU bytes are the reference, the destination arena is prefilled so
an unwritten byte cannot match, and the whole arena (guards included) is
compared. No tolerances.

`stream_threshold=1` sends any 16 B bulk down the streaming kernel and
`stream_blocks` caps its grid, so a few tens of KiB reach every path: with
stream_blocks=2 workgroup 0 takes tiles 0, 2, 4, ... and workgroup 1 takes
1, 3, 5, ...; the ragged last tile runs the bounds-checked body.

Sizes are written for U=4 (tile = 1024 elements of 16 B) and scaled by the
production U, so they keep their position relative to the tile.
"""
import itertools

import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from starway_amd import _core  # noqa: E402

from _guard import GuardedCopy, Region  # noqa: E402

STREAM = _core._copy_stream_tuning()
U = STREAM["unroll"]
K = U // 4            # scale of the U=4 sizes below
TILE = 256 * U        # elements of 16 B
NEVER = (1 << 64) - 1  # stream_threshold that no message reaches

N16 = [
    1,                # ragged tile only, one lane
    1023,             # ragged tile only, one element short of a full tile
    1024,             # exactly one full tile, no ragged body
    1025,             # one full tile (block 0) + 1 ragged element (block 1)
    2048,             # one full tile per block
    2049,             # two full tiles + ragged tile back on block 0
    3072,             # block 0 takes two tiles, block 1 one
    4 * 1024 + 513,   # two full tiles each + ragged on block 0
    7 * 1024 + 1023,  # 4 + 3 full tiles, ragged on block 1
]
OFFSETS = [0, 1, 15]
TAILS = [0, 1, 15]


def _run_flat(seed, src_off, dst_off, nbytes, label, **tuning):
    case = GuardedCopy(seed, Region.flat(src_off, nbytes),
                       Region.flat(dst_off, nbytes))
    _core._copy_device_sync(case.dst_ptr, case.src_ptr, nbytes, 0, **tuning)
    case.check(label)


def _scaled(n16):
    # 1 stays one element; everything else keeps its tile-relative position.
    return n16 if n16 == 1 else n16 * K


@pytest.mark.parametrize("n16", N16)
def test_stream_two_blocks(n16):
    """stream_blocks=2, every bulk size crossed with byte offsets {0,1,15}
    (head of 0, 15, 1 bytes through k_copy_elem<1>) and tails {0,1,15}."""
    n = _scaled(n16)
    for k, (off, tail) in enumerate(itertools.product(OFFSETS, TAILS)):
        head = (16 - off) % 16
        nbytes = head + n * 16 + tail
        _run_flat(7000 + n16 * 16 + k, off, off, nbytes,
                  f"k_copy_stream U={U} n16={n} off={off} tail={tail}",
                  stream_threshold=1, stream_blocks=2)


def test_stream_single_block():
    """stream_blocks=1: one workgroup walks five full tiles and a ragged
    one; odd head and tail."""
    n16 = 5 * TILE + TILE // 2 + 7
    _run_flat(7100, 9, 9, 7 + n16 * 16 + 5, f"k_copy_stream U={U} blocks=1",
              stream_threshold=1, stream_blocks=1)


def test_stream_grid_larger_than_tiles():
    """A cap far above the tile count: the grid is the tile count and each
    workgroup takes one tile, the last one ragged."""
    n16 = 3 * TILE + 77
    _run_flat(7150, 0, 0, n16 * 16 + 3, f"k_copy_stream U={U} uncapped",
              stream_threshold=1, stream_blocks=1 << 40)


@pytest.mark.parametrize("delta", [-16, 0], ids=["below", "at"])
def test_route_around_explicit_threshold(delta):
    """A bulk 16 bytes below an explicit stream_threshold takes the old
    route, at it the streaming kernel; both byte-exact. Offset 3 gives a
    13-byte head, and there is a 5-byte tail."""
    threshold = 3 * TILE * 16 + 16 * 40
    bulk = threshold + delta
    _run_flat(7200 + delta, 3, 3, 13 + bulk + 5,
              f"stream_threshold={threshold} bulk={bulk}",
              block_cap=2, stream_threshold=threshold, stream_blocks=2)


@pytest.mark.parametrize("nbytes", [1025 * 16, 40_000])
def test_not_coaligned_keeps_old_kernels(nbytes):
    """src and dst not co-aligned (offsets 1 and 2): the streaming route
    does not apply whatever the threshold; the byte kernel runs, exact."""
    _run_flat(7300 + nbytes, 1, 2, nbytes, "offsets 1/2 under stream tuning",
              block_cap=2, stream_threshold=1, stream_blocks=2)


def test_default_tuning_smallest_streamed_size():
    """Default tuning at one default stream_threshold plus 64 KiB: the
    smallest size class that takes the new route by default, with a 5-byte
    offset (11-byte head) and a 21-byte tail. The only large case. Where
    the default leaves the streaming kernel off (no threshold any message
    reaches), there is no such size and the explicit-tuning cases above are
    the coverage."""
    threshold = STREAM["stream_threshold"]
    if threshold >= 1 << 40:
        assert threshold == NEVER
        return
    nbytes = 11 + threshold + (64 << 10) + 21
    _run_flat(7400, 5, 5, nbytes,
              f"default tuning, {threshold} + 64 KiB + head/tail")
