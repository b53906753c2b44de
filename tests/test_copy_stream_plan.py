"""Host-only checks of the streaming copy's tile plan (csrc/copy_stream.hpp),
through `_core._copy_stream_plan`. Workgroup b of a grid of G takes tiles
b, b+G, b+2G, ...; the last tile may be ragged. Over all workgroups the
tiles must cover [0, n16) exactly once, with nothing past the end.

Small counts are enumerated element by element; large ones are checked in
closed form with Python integers, which do not wrap.
"""
import numpy as np
import pytest

from starway_amd import _core

TILE = 256 * _core._copy_stream_tuning()["unroll"]
K = TILE // 1024  # the sizes below are written for U=4 (tile 1024)

SMALL_N16 = [1, 1023, 1024, 1025, 2048, 2049, 3 * 1024, 4 * 1024 + 513,
             7 * 1024 + 1023]
if K > 1:  # the same tile-relative positions at the production tile size
    SMALL_N16 += [n * K for n in SMALL_N16[1:]] + [TILE - 1, TILE + 1]
LARGE_N16 = [2**32 - 1, 2**32, 2**32 + 1025, 2**40 + 7]


def _plan(n16, blocks, block=None):
    return _core._copy_stream_plan(n16, blocks, block)


def _expect_header(n16, blocks):
    full, ragged = divmod(n16, TILE)
    tiles = full + (1 if ragged else 0)
    return {"tile": TILE, "full_tiles": full, "ragged": ragged,
            "tiles": tiles, "grid": min(tiles, blocks)}


@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("n16", SMALL_N16)
def test_small_counts_cover_exactly_once(n16, blocks):
    p = _plan(n16, blocks)
    assert p == _expect_header(n16, blocks)
    assert p["grid"] >= 1
    hits = np.zeros(n16 + TILE, dtype=np.int32)  # room to see an overrun
    owned = 0
    for b in range(p["grid"]):
        pb = _plan(n16, blocks, b)
        assert pb["first_tile"] == b
        assert pb["n_tiles"] >= 1
        assert pb["last_tile"] == b + (pb["n_tiles"] - 1) * p["grid"]
        assert pb["last_tile"] < p["tiles"]
        assert pb["last_tile"] + p["grid"] >= p["tiles"]  # nothing skipped
        for t in range(pb["first_tile"], pb["last_tile"] + 1, p["grid"]):
            lo = t * TILE
            hi = lo + (TILE if t < p["full_tiles"] else p["ragged"])
            hits[lo:hi] += 1
        owned += pb["n_tiles"]
    assert owned == p["tiles"]
    assert (hits[:n16] == 1).all()
    assert (hits[n16:] == 0).all()
    # A workgroup past the grid owns nothing.
    assert _plan(n16, blocks, p["grid"])["n_tiles"] == 0


@pytest.mark.parametrize("n16", SMALL_N16)
def test_small_counts_8192_blocks_against_numpy_model(n16):
    blocks = 8192
    p = _plan(n16, blocks)
    assert p == _expect_header(n16, blocks)
    # Model: tile t belongs to workgroup t % grid.
    t = np.arange(p["tiles"], dtype=np.int64)
    owner = t % p["grid"]
    for b in range(p["grid"]):
        mine = t[owner == b]
        pb = _plan(n16, blocks, b)
        assert (pb["first_tile"], pb["last_tile"], pb["n_tiles"]) == (
            int(mine[0]), int(mine[-1]), mine.size)
    lens = np.full(p["tiles"], TILE, dtype=np.int64)
    if p["ragged"]:
        lens[-1] = p["ragged"]
    assert int(lens.sum()) == n16
    assert int(t[-1]) * TILE + int(lens[-1]) == n16  # ends exactly at n16


@pytest.mark.parametrize("blocks", [1, 2, 3, 8192])
@pytest.mark.parametrize("n16", LARGE_N16)
def test_large_counts_closed_form(n16, blocks):
    p = _plan(n16, blocks)
    assert p == _expect_header(n16, blocks)
    tiles, grid = p["tiles"], p["grid"]
    assert grid == blocks  # far more tiles than workgroups
    # The last element's byte offset does not fit 32 bits, and for 2**40 the
    # element index does not either.
    assert (n16 - 1) * 16 >= 2**32
    total = 0
    for b in sorted({0, 1 % grid, grid // 2, grid - 1,
                     (tiles - 1) % grid, p["full_tiles"] % grid}):
        pb = _plan(n16, blocks, b)
        count = (tiles - b + grid - 1) // grid
        assert pb["first_tile"] == b
        assert pb["n_tiles"] == count
        assert pb["last_tile"] == b + (count - 1) * grid
        assert pb["last_tile"] < tiles
        assert pb["last_tile"] * TILE < n16  # starts inside the message
    # Every workgroup's count, summed in closed form, is the tile count:
    # the first (tiles % grid) workgroups hold one tile more.
    q, r = divmod(tiles, grid)
    for b, count in ((0, q + (1 if r else 0)), (grid - 1, q)):
        assert _plan(n16, blocks, b)["n_tiles"] == count
    total = r * (q + 1) + (grid - r) * q
    assert total == tiles
    assert p["full_tiles"] * TILE + p["ragged"] == n16
    # The ragged tile is the last one and exactly one workgroup holds it.
    if p["ragged"]:
        holder = p["full_tiles"] % grid
        assert _plan(n16, blocks, holder)["last_tile"] == p["full_tiles"]


def test_default_stream_blocks_and_hooks_agree():
    t = _core._copy_stream_tuning()
    assert set(t) == {"stream_threshold", "stream_blocks", "unroll"}
    assert t["unroll"] in (4, 8)
    assert t["stream_blocks"] >= 1
    # stream_blocks=0 means the process default.
    assert _plan(10 * TILE * t["stream_blocks"], 0) == _plan(
        10 * TILE * t["stream_blocks"], t["stream_blocks"])
    assert set(_core._copy_tuning()) == {"block_cap", "nt_threshold",
                                         "nt_unroll"}
