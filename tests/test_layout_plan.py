"""Host tests of the N-D layout normalisation (csrc/layout.hpp) through the
_core._plan_layout / _core._plan_granule hooks. No GPU needed.

The reference is numpy: as_strided over an arena that holds each byte's own
offset enumerates a view's bytes in C order.
"""
import itertools

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

from starway_amd import _core

MAX_DIMS = 5


def plan_offsets(unit, dims):
    """Byte offsets, in message order, that a plan describes."""
    offs = np.zeros(1, dtype=np.int64)
    for extent, stride in dims:
        offs = (offs[:, None]
                + np.arange(extent, dtype=np.int64) * stride).reshape(-1)
    return (offs[:, None] + np.arange(unit, dtype=np.int64)).reshape(-1)


def numpy_offsets(shape, strides, itemsize, span):
    """The same from numpy: view an arena of byte offsets."""
    idx = np.arange(span, dtype=np.int64)
    v = as_strided(idx, tuple(shape) + (itemsize,),
                   tuple(8 * s for s in strides) + (8,))
    return v.reshape(-1)


def span_of(shape, strides, itemsize):
    return sum((e - 1) * s for e, s in zip(shape, strides)) + itemsize


def random_view(rng):
    """A numpy view built the way users build them: a dense base, a slice
    with steps, a permutation, sometimes a size-1 or a stride-0 dimension."""
    ndim = int(rng.integers(1, 7))
    itemsize = int(rng.choice([1, 2, 4, 8, 16]))
    extents = [int(rng.integers(1, 6)) for _ in range(ndim)]
    steps = [int(rng.integers(1, 4)) if rng.random() < 0.4 else 1
             for _ in range(ndim)]
    slack = [int(rng.integers(0, 3)) if rng.random() < 0.4 else 0
             for _ in range(ndim)]
    base = np.zeros([e * st + sl for e, st, sl in zip(extents, steps, slack)],
                    dtype=f"V{itemsize}")
    v = base[tuple(slice(0, e * st, st) for e, st in zip(extents, steps))]
    if rng.random() < 0.6:
        v = v.transpose(rng.permutation(ndim))
    if rng.random() < 0.25:
        d = int(rng.integers(0, ndim))
        v = v[tuple(slice(0, 1) if i == d else slice(None)
                    for i in range(ndim))]
        if rng.random() < 0.6:  # expand(): stride 0 over extent > 1
            shape = list(v.shape)
            shape[d] = int(rng.integers(2, 5))
            v = np.broadcast_to(v, shape)
    return v.shape, v.strides, itemsize


def test_offsets_match_numpy_for_seeded_views():
    rng = np.random.default_rng(20240)
    planned = rejected = 0
    seen_itemsize, seen_stride0, seen_ndim = set(), 0, set()
    for _ in range(400):
        shape, strides, itemsize = random_view(rng)
        try:
            unit, dims = _core._plan_layout(list(shape), list(strides),
                                            itemsize)
        except ValueError as e:
            # Only the dimension limit can refuse a forward-strided view,
            # and only a view with more than MAX_DIMS real dimensions.
            assert "dimensions" in str(e)
            assert sum(1 for e_ in shape if e_ > 1) > MAX_DIMS
            rejected += 1
            continue
        planned += 1
        assert len(dims) <= MAX_DIMS
        assert all(e > 1 for e, _ in dims), "size-1 dimension kept"
        want = numpy_offsets(shape, strides, itemsize,
                             span_of(shape, strides, itemsize))
        got = plan_offsets(unit, dims)
        assert np.array_equal(got, want), (shape, strides, itemsize, unit,
                                           dims)
        seen_itemsize.add(itemsize)
        seen_ndim.add(len(shape))
        seen_stride0 += any(s == 0 and e > 1 for e, s in zip(shape, strides))
    # The generator reached what it is meant to reach.
    assert planned >= 300 and rejected >= 1
    assert seen_itemsize == {1, 2, 4, 8, 16}
    assert seen_ndim == {1, 2, 3, 4, 5, 6}
    assert seen_stride0 >= 10


@pytest.mark.parametrize("itemsize", [1, 2, 4, 8, 16])
def test_contiguous_is_ndim_zero(itemsize):
    shape = (3, 1, 4, 5)
    strides = (20 * itemsize, 999, 5 * itemsize, itemsize)  # size-1: any
    unit, dims = _core._plan_layout(list(shape), list(strides), itemsize)
    assert dims == [] and unit == 60 * itemsize


def test_mergeable_dimensions_merge():
    # (4,3,5,6) fp32 rows of 6 in a pitch of 8; dims 1 and 2 merge.
    unit, dims = _core._plan_layout([4, 3, 5, 6], [1000, 160, 32, 4], 4)
    assert (unit, dims) == (24, [(4, 1000), (15, 32)])
    # A transposed matrix keeps both dimensions and single elements.
    unit, dims = _core._plan_layout([6, 10], [2, 12], 2)
    assert (unit, dims) == (2, [(6, 2), (10, 12)])
    # expand() of two leading dimensions: both stride 0, merged.
    unit, dims = _core._plan_layout([2, 3, 8], [0, 0, 1], 1)
    assert (unit, dims) == (8, [(6, 0)])
    # One strided dimension over a dense run: today's 2-D layout.
    unit, dims = _core._plan_layout([2, 4, 16], [256, 64, 2], 2)
    assert (unit, dims) == (32, [(8, 64)])
    # No elements.
    assert _core._plan_layout([3, 0, 2], [8, 8, 4], 4) == (0, [])


def test_limits_raise_value_error():
    # Six dimensions none of which merge.
    shape = [2] * 6
    strides = [3 ** (6 - i) * 4 for i in range(6)]
    with pytest.raises(ValueError, match="dimensions"):
        _core._plan_layout(shape, strides, 4)
    # ...but five are fine, and so are six once two of them merge.
    assert len(_core._plan_layout(shape[1:], strides[1:], 4)[1]) == 5
    merged = strides[:4] + [16, 8]
    assert len(_core._plan_layout(shape, merged, 4)[1]) == 5
    with pytest.raises(ValueError, match="negative"):
        _core._plan_layout([4, 4], [-16, 4], 4)
    # Destinations must not overlap; the same views are legal sources.
    for shape, strides in [
        ([3, 8], [0, 1]),          # stride 0 over extent 3
        ([4, 8], [4, 1]),          # rows 8 long, 4 apart
        ([3, 4, 2], [8, 2, 16]),   # dim 2 lands inside dims 0/1's extent
    ]:
        _core._plan_layout(shape, strides, 1)
        with pytest.raises(ValueError, match="overlap"):
            _core._plan_layout(shape, strides, 1, writable=True)
    # A transposed destination does not overlap.
    _core._plan_layout([6, 10], [2, 12], 2, writable=True)


QUANTITIES = ["src_ptr", "dst_ptr", "src_stride", "dst_stride", "src_unit",
              "dst_unit"]


def granule_case(which=None, g=16):
    """Everything a multiple of 16 except `which`, whose lowest set bit is
    g. Returns the arguments of _plan_granule."""
    q = {"src_ptr": 4096, "dst_ptr": 8192, "src_stride": 96,
         "dst_stride": 160, "src_unit": 48, "dst_unit": 80}
    if which is not None:
        q[which] = q[which] + 48 + g  # 48 + g: lowest set bit is g
    src = (q["src_unit"], [(3, 4096), (5, q["src_stride"])])
    dst = (q["dst_unit"], [(3, q["dst_stride"])])
    return src, dst, q["src_ptr"], q["dst_ptr"]


def test_granule_baseline_is_16():
    assert _core._plan_granule(*granule_case()) == 16


@pytest.mark.parametrize("which,g",
                         list(itertools.product(QUANTITIES, [8, 4, 2, 1])))
def test_granule_drops_for_one_quantity(which, g):
    assert _core._plan_granule(*granule_case(which, g)) == g
