"""Argument contract of the reducing receive (``reduce="sum"``), as far as
it shows without a device: what is refused when the receive is posted, and
that a plain receive is what it was."""
import contextlib

import numpy as np
import pytest

from starway_amd import Client, Server, _core

SERVER_ADDR = "127.0.0.1"
FULL = (1 << 64) - 1


@contextlib.asynccontextmanager
async def pair(port):
    server = Server()
    client = Client()
    server.listen(SERVER_ADDR, port)
    await client.aconnect(SERVER_ADDR, port)
    try:
        yield server, client
    finally:
        await client.aclose()
        await server.aclose()


class Untouchable:
    """Any look at this object as a buffer fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"buffer touched ({name}) before the op check")


def _never(*_):
    raise AssertionError("callback of a receive that was never posted")


async def test_reduce_on_a_host_buffer_is_refused(port):
    async with pair(port) as (server, client):
        buf = np.zeros(16, dtype=np.float32)
        for end in (server, client):
            with pytest.raises(ValueError, match="host"):
                end.arecv(buf, 0, 0, reduce="sum")
            with pytest.raises(ValueError, match="host"):
                end.recv(buf, 0, 0, _never, _never, reduce="sum")
        # The native layer refuses it too, whatever dtype it is told.
        with pytest.raises(ValueError, match="host"):
            server._server.recv(buf, 0, 0, _never, _never, reduce="sum",
                                dtype="float32")
        with pytest.raises(ValueError, match="host"):
            client._client.recv(buf, 0, 0, _never, _never, reduce="sum",
                                dtype="float32")
        assert not buf.any()


async def test_unknown_op_is_refused_before_the_buffer_is_touched(port):
    async with pair(port) as (server, client):
        for end in (server, client):
            with pytest.raises(ValueError, match="max"):
                end.arecv(Untouchable(), 0, 0, reduce="max")
            with pytest.raises(ValueError, match="max"):
                end.recv(Untouchable(), 0, 0, _never, _never, reduce="max")
        with pytest.raises(ValueError, match="max"):
            server._server.recv(Untouchable(), 0, 0, _never, _never,
                                reduce="max", dtype="float32")
        with pytest.raises(ValueError, match="max"):
            client._client.recv(Untouchable(), 0, 0, _never, _never,
                                reduce="max", dtype="float32")


async def test_plain_recv_is_unchanged_and_counts_no_reduce(port):
    async with pair(port) as (server, client):
        buf = np.zeros(64, dtype=np.uint8)
        fut = server.arecv(buf, 5, FULL)
        await server.aflush()
        await client.asend(np.arange(64, dtype=np.uint8), 5)
        assert tuple(await fut) == (5, 64)
        assert (buf == np.arange(64)).all()
        # reduce=None is the plain receive as well.
        back = np.zeros(8, dtype=np.uint8)
        fut = client.arecv(back, 0, 0, reduce=None)
        ep = next(iter(server.list_clients()))
        await server.asend(ep, np.full(8, 3, dtype=np.uint8), 6)
        assert tuple(await fut) == (6, 8)
        assert (back == 3).all()
        for stats in (server._server.get_stats(), client._client.get_stats()):
            assert stats["reduce_rx"] == 0


def test_accum_hook_refuses_what_the_kernels_cannot_take():
    """Checked before any device is touched."""
    with pytest.raises(ValueError, match="dtype"):
        _core._accum_sync(256, 512, 16, "float64", 0)
    with pytest.raises(ValueError, match="dtype"):
        _core._accum_sync(256, 512, 16, "uint8", 0)
    with pytest.raises(ValueError, match="item size"):
        _core._accum_sync(256, 512, 6, "float32", 0)
    with pytest.raises(ValueError, match="item size"):
        _core._accum_sync(258, 512, 8, "int32", 0)
    with pytest.raises(ValueError, match="item size"):
        _core._accum_sync(256, 513, 8, "bfloat16", 0)
