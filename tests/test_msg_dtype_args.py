"""Argument contract of the converting receive (``msg_dtype=``), as far as
it shows without a device: what is refused when the receive is posted, that
a plain receive is what it was, and how the convert dispatch splits a
message (``_core._convert_plan``, host only)."""
import contextlib

import numpy as np
import pytest

from starway_amd import Client, Server, _core

SERVER_ADDR = "127.0.0.1"
FULL = (1 << 64) - 1
ES = {"float32": 4, "float16": 2, "bfloat16": 2}


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
        raise AssertionError(f"buffer touched ({name}) before the name check")


def _never(*_):
    raise AssertionError("callback of a receive that was never posted")


def natives(server, client):
    return server._server, client._client


@pytest.mark.parametrize("name", ["float8", "int32", "float64", "uint8"])
async def test_bad_name_is_refused_before_the_buffer_is_touched(port, name):
    async with pair(port) as (server, client):
        for end in (server, client):
            with pytest.raises(ValueError, match="^msg_dtype limit:") as e:
                end.arecv(Untouchable(), 0, 0, msg_dtype=name)
            assert name in str(e.value)
            with pytest.raises(ValueError, match="^msg_dtype limit:"):
                end.recv(Untouchable(), 0, 0, _never, _never, msg_dtype=name)
            with pytest.raises(ValueError, match="^msg_dtype limit:"):
                end.arecv(Untouchable(), 0, 0, reduce="sum", msg_dtype=name)
        for native in natives(server, client):
            with pytest.raises(ValueError, match="^msg_dtype limit:") as e:
                native.recv(Untouchable(), 0, 0, _never, _never,
                            dtype="float32", msg_dtype=name)
            assert name in str(e.value)


async def test_a_torch_dtype_names_itself(port):
    torch = pytest.importorskip("torch")
    async with pair(port) as (server, client):
        with pytest.raises(ValueError, match="^msg_dtype limit:.*int32"):
            server.arecv(Untouchable(), 0, 0, msg_dtype=torch.int32)
        # A supported one gets as far as the buffer: a host buffer here.
        with pytest.raises(ValueError, match="^msg_dtype limit:.*host"):
            server.arecv(np.zeros(4, np.float32), 0, 0,
                         msg_dtype=torch.bfloat16)


async def test_a_host_buffer_is_refused(port):
    async with pair(port) as (server, client):
        buf = np.zeros(16, dtype=np.float32)
        for end in (server, client):
            with pytest.raises(ValueError, match="^msg_dtype limit:.*host"):
                end.arecv(buf, 0, 0, msg_dtype="bfloat16")
            with pytest.raises(ValueError, match="^msg_dtype limit:.*host"):
                end.recv(buf, 0, 0, _never, _never, msg_dtype="float16")
        for native in natives(server, client):
            with pytest.raises(ValueError, match="^msg_dtype limit:.*host"):
                native.recv(buf, 0, 0, _never, _never, dtype="float32",
                            msg_dtype="bfloat16")
        assert not buf.any()


async def test_index_with_msg_dtype_is_refused(port):
    async with pair(port) as (server, client):
        buf = np.zeros((4, 4), dtype=np.float32)
        for end in (server, client):
            with pytest.raises(ValueError, match="^msg_dtype limit:.*index"):
                end.arecv(buf, 0, 0, index=[0, 1], msg_dtype="bfloat16")
            with pytest.raises(ValueError, match="^msg_dtype limit:.*index"):
                end.recv(buf, 0, 0, _never, _never, index=[0, 1],
                         msg_dtype="bfloat16")
        for native in natives(server, client):
            with pytest.raises(ValueError, match="^msg_dtype limit:.*index"):
                native.recv(buf, 0, 0, _never, _never, dtype="float32",
                            index=[0, 1], msg_dtype="bfloat16")


async def test_plain_recv_is_unchanged_and_counts_no_cast(port):
    async with pair(port) as (server, client):
        buf = np.zeros(64, dtype=np.uint8)
        fut = server.arecv(buf, 5, FULL)
        await server.aflush()
        await client.asend(np.arange(64, dtype=np.uint8), 5)
        assert tuple(await fut) == (5, 64)
        assert (buf == np.arange(64)).all()
        # msg_dtype=None is the plain receive as well.
        back = np.zeros(8, dtype=np.uint8)
        fut = client.arecv(back, 0, 0, msg_dtype=None)
        ep = next(iter(server.list_clients()))
        await server.asend(ep, np.full(8, 3, dtype=np.uint8), 6)
        assert tuple(await fut) == (6, 8)
        assert (back == 3).all()
        # So is the native form with its default.
        raw = np.zeros(8, dtype=np.uint8)
        done = []
        server._server.recv(raw, 7, FULL, lambda *a: done.append(a), _never,
                            msg_dtype="")
        await server.aflush()
        await client.asend(np.full(8, 9, dtype=np.uint8), 7)
        flag = np.zeros(1, dtype=np.uint8)
        fut = server.arecv(flag, 8, FULL)
        await client.asend(np.ones(1, dtype=np.uint8), 8)
        await fut
        assert done == [(7, 8)] and (raw == 9).all()
        for stats in (server._server.get_stats(), client._client.get_stats()):
            assert stats["cast_rx"] == 0
            assert stats["reduce_rx"] == 0


def test_convert_hooks_refuse_what_the_kernels_cannot_take():
    """Checked before any device is touched."""
    with pytest.raises(ValueError, match="dtype"):
        _core._convert_sync(256, 512, 4, "float32", "int32", 0)
    with pytest.raises(ValueError, match="dtype"):
        _core._convert_sync(256, 512, 4, "float64", "float32", 0)
    with pytest.raises(ValueError, match="equal"):
        _core._convert_sync(256, 512, 4, "float16", "float16", 0)
    with pytest.raises(ValueError, match="item size"):
        _core._convert_sync(258, 512, 4, "float32", "bfloat16", 0)
    with pytest.raises(ValueError, match="item size"):
        _core._convert_sync(256, 513, 4, "float32", "bfloat16", 0)
    with pytest.raises(ValueError, match="shape"):
        _core._convert_sync(256, 512, 4, "float32", "bfloat16", 0, shape="c")
    with pytest.raises(ValueError, match="non-temporal"):
        _core._convert_sync(256, 512, 4, "float32", "bfloat16", 0,
                            nt_threshold=1)
    with pytest.raises(TypeError):  # the tuning is keyword-only
        _core._convert_sync(256, 512, 4, "float32", "bfloat16", 0, True)
    with pytest.raises(ValueError, match="shape"):
        _core._convert_plan(256, 512, 4, "float32", "bfloat16", "x")


def _expected_plan(dst, ds, src, ss, n, lane_elems):
    """Smallest head that puts both sides on their access boundary, found
    by trying every head; None when there is none."""
    src_access = min(16, lane_elems * ss)
    dst_access = min(16, lane_elems * ds)
    for h in range(64):  # far past the period of either side
        if (src + h * ss) % src_access == 0 and (dst + h * ds) % dst_access == 0:
            head = min(h, n)
            return {"kernel": "vector", "lane_elems": lane_elems,
                    "head": head, "vectors": (n - head) // lane_elems,
                    "tail": (n - head) % lane_elems}
    return {"kernel": "element", "lane_elems": lane_elems, "head": 0,
            "vectors": 0, "tail": n}


@pytest.mark.parametrize("dst_dtype,src_dtype,shape,lane_elems", [
    ("float32", "bfloat16", "a", 8),
    ("float32", "bfloat16", "b", 4),
    ("float16", "float32", "a", 8),
    ("float16", "float32", "b", 4),
    ("float16", "bfloat16", "a", 8),
    ("float16", "bfloat16", "b", 8),  # 2 <-> 2 has one shape
])
def test_dispatch_plan_for_every_offset_pair(dst_dtype, src_dtype, shape,
                                             lane_elems):
    ds, ss = ES[dst_dtype], ES[src_dtype]
    kinds = set()
    for n in (1000, 3, 0):
        for so in range(8):
            for do in range(8):
                src = (1 << 20) + so * ss
                dst = (1 << 21) + do * ds
                want = _expected_plan(dst, ds, src, ss, n, lane_elems)
                got = _core._convert_plan(dst, src, n, dst_dtype, src_dtype,
                                          shape)
                assert got == want, (so, do, n, got, want)
                assert got["head"] + lane_elems * got["vectors"] + \
                    got["tail"] == n
                kinds.add(got["kernel"])
    assert kinds == {"vector", "element"}


def test_the_production_shape_is_one_of_the_two():
    prod = _core._convert_shape()
    assert prod in ("a", "b")
    other = "a" if prod == "b" else "b"
    try:
        assert _core._convert_shape(other) == other
        plan = _core._convert_plan(1 << 21, 1 << 20, 64, "float32",
                                   "bfloat16")
        assert plan["lane_elems"] == {"a": 8, "b": 4}[other]
    finally:
        assert _core._convert_shape("") == prod
    plan = _core._convert_plan(1 << 21, 1 << 20, 64, "float32", "bfloat16")
    assert plan["lane_elems"] == {"a": 8, "b": 4}[prod]
