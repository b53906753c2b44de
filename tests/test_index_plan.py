"""Indexed send/recv, everything that needs no device: the index limits at
post time (facade and _core, Server and Client), the host-only hooks
_plan_index / _index_offset, the FT_RTS_INDEXED payload round trip and its
malformed forms, the argument checks of _copy_index_sync, and index=None
leaving a plain host transfer as it was.
"""
import asyncio

import numpy as np
import pytest

import starway_amd as sw
from starway_amd import _core

HOST_POOL = np.zeros((8, 16), dtype=np.uint8)


def _noop(*_a):
    pass


def _posters():
    """Every way to post an indexed operation, as (label, post(buf, index)).
    None of them needs a connection: a limit is raised before the engine
    sees the operation."""
    server, client = sw.Server(), sw.Client()
    return [
        ("Server.send", lambda b, i: server.send(None, b, 1, _noop, _noop,
                                                 index=i)),
        ("Server.recv", lambda b, i: server.recv(b, 1, 0, _noop, _noop,
                                                 index=i)),
        ("Client.send", lambda b, i: client.send(b, 1, _noop, _noop,
                                                 index=i)),
        ("Client.recv", lambda b, i: client.recv(b, 1, 0, _noop, _noop,
                                                 index=i)),
        ("_core.Server.send", lambda b, i: server._server.send(
            None, b, 1, _noop, _noop, index=i)),
        ("_core.Server.recv", lambda b, i: server._server.recv(
            b, 1, 0, _noop, _noop, index=i)),
        ("_core.Client.send", lambda b, i: client._client.send(
            b, 1, _noop, _noop, index=i)),
        ("_core.Client.recv", lambda b, i: client._client.recv(
            b, 1, 0, _noop, _noop, index=i)),
    ]


LIMITS = [
    ("host buffer", [1, 2], "host buffers"),
    ("bool list", [True, False], "bool"),
    ("bool array", np.array([True, False]), "bool"),
    ("float list", [1.0, 2.0], "float"),
    ("float array", np.array([1.0, 2.0]), "float"),
    ("2-D list", [[1, 2], [3, 4]], "1-D"),
    ("2-D array", np.array([[1, 2], [3, 4]]), "1-D"),
    ("out of range", [1, 8], "out of range"),
    ("negative", [1, -1], "negative"),
]


@pytest.mark.parametrize("name,index,match", LIMITS,
                         ids=[c[0] for c in LIMITS])
def test_limits_raise_at_post_time(name, index, match):
    for label, post in _posters():
        with pytest.raises(ValueError, match=match) as exc:
            post(HOST_POOL, index)
        assert str(exc.value).startswith("index limit:"), (label, exc.value)


def test_async_facade_raises_at_post_time():
    async def inner():
        server, client = sw.Server(), sw.Client()
        with pytest.raises(ValueError, match="index limit: .*negative"):
            client.asend(HOST_POOL, 1, index=[-1])
        with pytest.raises(ValueError, match="index limit: .*host buffers"):
            server.arecv(HOST_POOL, 1, 0, index=[0])
        with pytest.raises(ValueError, match="index limit: .*reduce"):
            server.arecv(HOST_POOL, 1, 0, index=[0], reduce="sum")
        with pytest.raises(ValueError, match="index limit: .*reduce"):
            client._client.recv(HOST_POOL, 1, 0, _noop, _noop, reduce="sum",
                                dtype="float32", index=[0])

    asyncio.run(inner())


def test_cpu_torch_buffer_and_index_forms():
    torch = pytest.importorskip("torch")
    client = sw.Client()
    with pytest.raises(ValueError, match="index limit: .*host buffers"):
        client.send(torch.zeros(8, 16), 1, _noop, _noop,
                    index=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="index limit: .*bool"):
        client.send(torch.zeros(8, 16), 1, _noop, _noop,
                    index=torch.tensor([True]))
    assert _core._plan_index(torch.tensor([3, 0], dtype=torch.int32), 4) \
        == [3, 0]


def test_plan_index_forms_and_repeats():
    assert _core._plan_index([7, 0, 31, 4], 32, True) == [7, 0, 31, 4]
    assert _core._plan_index((2, 1), 3) == [2, 1]
    for dt in (np.int8, np.uint8, np.int32, np.int64, np.uint64):
        assert _core._plan_index(np.array([5, 0, 3], dtype=dt), 6, True) \
            == [5, 0, 3]
    assert _core._plan_index([], 0, True) == []
    with pytest.raises(ValueError, match="index limit: .*repeat"):
        _core._plan_index([7, 0, 10, 3, 3], 11, True)
    assert _core._plan_index([7, 0, 10, 3, 3], 11, False) \
        == [7, 0, 10, 3, 3]
    # The duplicate check does not depend on the pool's size.
    far = 2 ** 31
    assert _core._plan_index([5, far, 6], far + 1, True) == [5, far, 6]
    with pytest.raises(ValueError, match=f"index limit: .*repeat.*{far}"):
        _core._plan_index([far, 5, far], far + 1, True)
    dense_list = list(range(4096))
    assert _core._plan_index(dense_list, 4096, True) == dense_list
    with pytest.raises(ValueError, match="index limit: .*repeat.*4095"):
        _core._plan_index(dense_list + [4095], 4096, True)
    with pytest.raises(ValueError, match="index limit: .*out of range"):
        _core._plan_index(np.array([2 ** 63 + 5], dtype=np.uint64), 11)
    with pytest.raises(ValueError, match=r"index limit: .*2\*\*32"):
        _core._plan_index([0], 2 ** 32)
    with pytest.raises(ValueError, match="index limit: "):
        _core._plan_index("12", 4)


def test_plan_index_entry_limit():
    assert _core._INDEX_MAX == 65536
    full = np.arange(65536, dtype=np.int64)
    assert _core._plan_index(full, 65536, True) == full.tolist()
    over = np.zeros(65537, dtype=np.int64)
    with pytest.raises(ValueError, match="index limit: .*kIndexMax"):
        _core._plan_index(over, 65537, False)
    with pytest.raises(ValueError, match="index limit: .*kIndexMax"):
        _core._plan_index(over.tolist(), 65537, False)


def test_mutating_the_list_after_planning_changes_nothing():
    idx = [3, 1, 2]
    planned = _core._plan_index(idx, 4, True)
    idx[0] = 0
    assert planned == [3, 1, 2]


def _oracle_offset(index, slice_bytes, stride, m):
    return int(index[m // slice_bytes]) * stride + m % slice_bytes


def test_index_offset_matches_numpy():
    index = [7, 0, 10, 3, 9]
    pool = np.arange(11 * 1072, dtype=np.int64)  # byte offsets of a pool
    rows = np.lib.stride_tricks.as_strided(pool, (11, 1040), (1072 * 8, 8))
    message = rows[index].reshape(-1)  # offset of every message byte
    for m in (0, 1, 1039, 1040, 2079, 2080, 3 * 1040 + 517, 5 * 1040 - 1):
        got = _core._index_offset(index, 1040, 1072, m)
        assert got == int(message[m]) == _oracle_offset(index, 1040, 1072, m)
    with pytest.raises(ValueError):
        _core._index_offset(index, 1040, 1072, 5 * 1040)


def test_index_offset_is_64_bit():
    # idx * stride above 2**32: neither the stride nor the product fits 32
    # bits (the second product is 2**53 + 2**33, still inside 64).
    stride = 2 ** 33
    index = [3, 2 ** 20 + 1]
    assert _core._index_offset(index, 4096, stride, 100) == 3 * stride + 100
    assert _core._index_offset(index, 4096, stride, 4096 + 7) \
        == (2 ** 20 + 1) * stride + 7


DESC = bytes((i * 7 + 3) & 0xFF for i in range(_core._RTS_DESC_BYTES))


def test_descriptor_round_trip():
    assert _core._PROTO_VERSION == 4
    assert _core._FT_RTS_INDEXED == 17
    index = [7, 0, 10, 3, 3]
    payload = _core._index_desc_encode(DESC, index, 1040, 1072)
    assert len(payload) == len(DESC) + 24 + 4 * len(index)
    assert payload[:len(DESC)] == DESC  # RtsDesc travels unchanged
    head = np.frombuffer(payload[len(DESC):len(DESC) + 24], dtype="<u8")
    assert head[0] == 1040 and head[1] == 1072
    assert np.frombuffer(payload[len(DESC) + 16:len(DESC) + 24],
                         dtype="<u4").tolist() == [5, 0]
    assert np.frombuffer(payload[len(DESC) + 24:],
                         dtype="<u4").tolist() == index
    assert _core._index_desc_decode(payload, 5 * 1040) \
        == (index, 1040, 1072)
    empty = _core._index_desc_encode(DESC, [], 1040, 1072)
    assert _core._index_desc_decode(empty, 0) == ([], 1040, 1072)


def _payload(slice_bytes, stride, count, entries):
    return (DESC + np.array([slice_bytes, stride], dtype="<u8").tobytes()
            + np.array([count, 0], dtype="<u4").tobytes()
            + np.array(entries, dtype="<u4").tobytes())


def test_malformed_descriptors_are_refused():
    good = _payload(1040, 1072, 3, [7, 0, 3])
    assert _core._index_desc_decode(good, 3 * 1040) == ([7, 0, 3], 1040, 1072)
    # length disagrees with count: an entry short, an entry long, no header
    for bad in (good[:-4], good + b"\0\0\0\0", good[:len(DESC) + 10]):
        with pytest.raises(ValueError):
            _core._index_desc_decode(bad, 3 * 1040)
    # count > kIndexMax
    with pytest.raises(ValueError, match="kIndexMax"):
        _core._index_desc_decode(_payload(16, 16, 65537, [0] * 65537),
                                 65537 * 16)
    # count * slice_bytes != size
    with pytest.raises(ValueError, match="add up"):
        _core._index_desc_decode(good, 3 * 1040 - 16)
    with pytest.raises(ValueError, match="add up"):
        _core._index_desc_decode(_payload(2 ** 63, 0, 2, [0, 1]), 0)
    # slice_bytes == 0 with count > 0
    with pytest.raises(ValueError, match="empty slices"):
        _core._index_desc_decode(_payload(0, 16, 3, [7, 0, 3]), 0)


def test_copy_index_sync_checks_arguments_before_any_device():
    """Null pointers and device -1: reaching a device would fault or
    fail differently; a ValueError means the check came first."""
    hook = _core._copy_index_sync
    with pytest.raises(ValueError, match="both sides are dense"):
        hook(0, None, 0, 0, 0, None, 0, 0, 4096, -1)
    with pytest.raises(ValueError, match="destination slices hold"):
        hook(0, [1, 2], 1040, 1072, 0, None, 0, 0, 3 * 1040, -1)
    with pytest.raises(ValueError, match="source slices hold"):
        hook(0, None, 0, 0, 0, [1, 2, 2], 1040, 1072, 2 * 1040, -1)
    with pytest.raises(ValueError, match="source slices hold"):
        hook(0, [0, 1, 2, 3], 1152, 1152, 0, [1, 2, 0, 4, 5], 768, 768,
             4 * 1152, -1)
    with pytest.raises(ValueError, match="slice size or stride"):
        hook(0, [1, 2], 0, 16, 0, None, 0, 0, 0, -1)
    with pytest.raises(ValueError, match="slice size or stride"):
        hook(0, [1, 2], 32, 16, 0, None, 0, 0, 64, -1)  # overlapping
    with pytest.raises(ValueError, match="repeat"):
        hook(0, [1, 1], 16, 16, 0, None, 0, 0, 32, -1)


async def test_plain_host_transfer_is_unchanged():
    server, client = sw.Server(), sw.Client()
    await client.aconnect_address(server.listen_address())
    try:
        src = np.random.default_rng(7).integers(0, 256, 3000, dtype=np.uint8)
        dst = np.zeros(3000, dtype=np.uint8)
        fut = server.arecv(dst, 0, 0, index=None)
        await client.asend(src, 5, index=None)
        await client.aflush()
        assert await fut == (5, 3000)
        assert np.array_equal(dst, src)
        dst2 = np.zeros(3000, dtype=np.uint8)
        fut = server.arecv(dst2, 0, 0)
        await client.asend(src, 6)
        assert await fut == (6, 3000)
        assert np.array_equal(dst2, src)
        for stats in (server._server.get_stats(), client._client.get_stats()):
            assert stats["index_tx"] == 0 and stats["index_rx"] == 0
    finally:
        await client.aclose()
        await server.aclose()
