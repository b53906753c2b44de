"""The `_inbox_*` kernel hooks without a device: arguments are checked
before anything touches the GPU, and a build without one fails cleanly.

A detached `_InboxRing(slots, slot_bytes)` carries geometry only; it lets
the checks run anywhere and is refused by every call that would need
device memory. (The kernels themselves: tests/test_inbox_kernels.py.)"""
import pytest

import starway_amd
from starway_amd import _core


def test_inbox_hooks_validate_before_touching_a_device():
    ring = _core._InboxRing(64, 64 + 4096)
    assert (ring.slots, ring.slot_bytes, ring.hdr_bytes) == (64, 4160, 64)
    assert ring.payload_max == 4096
    assert not ring.live and ring.device == -1
    ok = (0x1000, 16, 1, 7)  # src, size, seq, tag

    # Batch size 1..32.
    for n in (0, 33):
        with pytest.raises(ValueError, match=r"1\.\.32"):
            _core._inbox_push_sync(ring, [ok] * n, 0)
        with pytest.raises(ValueError, match=r"1\.\.32"):
            _core._inbox_unpack_sync(ring, [(1, 16, 0)] * n)
    # size <= payload_max, anywhere in the batch.
    with pytest.raises(ValueError, match="payload_max"):
        _core._inbox_push_sync(ring, [ok, (0x1000, 4097, 2, 7)], 0)
    with pytest.raises(ValueError, match="payload_max"):
        _core._inbox_unpack_sync(ring, [(1, 4097, 0)])
    # seq 0 is the empty-slot sentinel.
    with pytest.raises(ValueError, match="seq 0"):
        _core._inbox_push_sync(ring, [(0x1000, 16, 0, 7)], 0)
    with pytest.raises(ValueError, match="seq 0"):
        _core._inbox_unpack_sync(ring, [(0, 16, 0)])
    with pytest.raises(ValueError, match="seq 0"):
        _core._inbox_arm_begin(ring, 0, 1, 1, 0x1000, 64)
    # Ring writes stay inside the ring.
    with pytest.raises(ValueError, match="out of range"):
        _core._inbox_ring_write(ring, 64 * 4160 - 1, b"ab")
    with pytest.raises(ValueError):
        _core._InboxRing(0, 4160)
    with pytest.raises(ValueError):
        _core._InboxRing(64, 63)

    # Valid arguments, but no device memory behind the ring.
    for call in (
        lambda: _core._inbox_push_sync(ring, [ok] * 32, 0),
        lambda: _core._inbox_unpack_sync(ring, [(1, 4096, 0)] * 32),
        lambda: _core._inbox_arm_begin(ring, 1, 1, 1, 0x1000, 64),
        lambda: _core._inbox_ring_read(ring),
        lambda: _core._inbox_ring_write(ring, 0, b"ab"),
        lambda: _core._inbox_ring_destroy(ring),
    ):
        with pytest.raises(RuntimeError, match="no device memory"):
            call()

    if not starway_amd.gpu_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            _core._inbox_ring_create(0)
