"""Receive-side counter contract of the host eager plane.

Rule under test: every delivered message counts exactly once in
``msgs_received`` / ``bytes_received`` / its plane counter (``eager_rx``
here), a message that arrived before its recv additionally counts once in
``unexpected_rx``, and a failed (truncated) delivery counts nowhere.

Ordering is made deterministic without sleeping: an engine processes its
command queue in order, so a completed ``aflush()`` on the receiver proves
every recv issued before it is posted; and one connection is one ordered
stream, so a delivered sentinel proves every earlier message was parsed.
"""
import contextlib

import numpy as np
import pytest

from starway_amd import Client, Server

SERVER_ADDR = "127.0.0.1"
FULL = (1 << 64) - 1
RX_KEYS = ("msgs_received", "bytes_received", "eager_rx", "unexpected_rx",
           "unexp_staged_bytes")


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


def rx_stats(server):
    st = server._server.get_stats()
    return {k: st[k] for k in RX_KEYS}


def delta(after, before):
    return {k: after[k] - before[k] for k in RX_KEYS}


async def test_preposted_eager_counts_once(port):
    async with pair(port) as (server, client):
        base = rx_stats(server)
        bufs = [np.zeros(64, dtype=np.uint8) for _ in range(3)]
        futs = [server.arecv(bufs[i], i, FULL) for i in range(3)]
        await server.aflush()  # recvs are posted once this returns
        for i in range(3):
            await client.asend(np.full(64, i + 1, dtype=np.uint8), i)
        for i, fut in enumerate(futs):
            tag, ln = await fut
            assert (tag, ln) == (i, 64)
            assert (bufs[i] == i + 1).all()
        assert delta(rx_stats(server), base) == {
            "msgs_received": 3, "bytes_received": 192, "eager_rx": 3,
            "unexpected_rx": 0, "unexp_staged_bytes": 0}


async def test_unexpected_eager_counts_once(port):
    async with pair(port) as (server, client):
        base = rx_stats(server)
        sentinel = np.zeros(1, dtype=np.uint8)
        sfut = server.arecv(sentinel, 99, FULL)
        await server.aflush()
        for i in range(3):
            await client.asend(np.full(64, i + 1, dtype=np.uint8), i)
        await client.asend(np.ones(1, dtype=np.uint8), 99)
        await client.aflush()
        await sfut  # the three messages ahead of it are parsed and staged
        staged = rx_stats(server)
        assert delta(staged, base) == {
            "msgs_received": 1, "bytes_received": 1, "eager_rx": 1,
            "unexpected_rx": 3, "unexp_staged_bytes": 192}
        for i in range(3):
            buf = np.zeros(64, dtype=np.uint8)
            tag, ln = await server.arecv(buf, i, FULL)
            assert (tag, ln) == (i, 64)
            assert (buf == i + 1).all()
        assert delta(rx_stats(server), staged) == {
            "msgs_received": 3, "bytes_received": 192, "eager_rx": 3,
            "unexpected_rx": 0, "unexp_staged_bytes": -192}
        assert rx_stats(server)["unexp_staged_bytes"] == 0


async def test_truncated_eager_counts_nothing(port):
    async with pair(port) as (server, client):
        base = rx_stats(server)
        small = np.zeros(64, dtype=np.uint8)
        fut = server.arecv(small, 0, 0)
        await server.aflush()
        await client.asend(np.full(128, 7, dtype=np.uint8), 1)
        with pytest.raises(Exception, match="truncated"):
            await fut
        assert delta(rx_stats(server), base) == dict.fromkeys(RX_KEYS, 0)
        # The connection survives and the next message counts once.
        buf = np.zeros(64, dtype=np.uint8)
        fut = server.arecv(buf, 0, 0)
        await server.aflush()
        await client.asend(np.full(64, 9, dtype=np.uint8), 2)
        tag, ln = await fut
        assert (tag, ln) == (2, 64)
        assert (buf == 9).all()
        assert delta(rx_stats(server), base) == {
            "msgs_received": 1, "bytes_received": 64, "eager_rx": 1,
            "unexpected_rx": 0, "unexp_staged_bytes": 0}
