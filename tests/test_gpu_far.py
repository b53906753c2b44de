"""Byte offsets past 2**31 and 2**32 through Server/Client: the wire fields
that carry them (RtsDesc::offset, src_stride, Layout::stride[],
IndexWire::stride) and the pull routes behind them, in same-process
loopback.

The buffers are as_strided views of the far arenas of tests/_guard_far.py
(a few KiB touched in 6.25 GiB; numpy expectation; every byte outside the
touched windows must keep its constant). The geometries are those of
tests/test_far_kernels.py. The module needs 32 GiB of free device memory
and skips as a whole below that.
"""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import starway_amd as sw  # noqa: E402

from _guard_far import (GUARD, NEED_FREE, PORCH, FarArenas, GuardedFar,  # noqa: E402
                        Pool, View, dense)

FULL = (1 << 64) - 1
GIB = 1 << 30


@pytest.fixture(scope="module")
def arenas():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"far arenas need {NEED_FREE >> 30} GiB of free device "
                    f"memory, {free >> 30} GiB are free")
    a = FarArenas()
    yield a
    a.src.buf = a.dst.buf = None
    torch.cuda.empty_cache()


@contextlib.asynccontextmanager
async def loopback():
    server = sw.Server()
    client = sw.Client()
    addr = server.listen_address()
    await client.aconnect_address(addr)
    try:
        yield server, client
    finally:
        await client.aclose()
        await server.aclose()


def far_case(arenas, seed, src, dst, far) -> GuardedFar:
    case = GuardedFar(arenas, seed, src, dst)
    for tag, side in (("s", src), ("d", dst)):
        assert case.crosses(side) == (tag in far), side
    return case


async def deliver(case: GuardedFar, tag: int, label: str):
    """client -> server, receive pre-posted."""
    async with loopback() as (server, client):
        fut = server.arecv(case.dst_view, tag, FULL, **case.dst_kw)
        await client.asend(case.src_view, tag, **case.src_kw)
        await client.aflush()
        assert await fut == (tag, case.src.nbytes), label
        case.check(label)
        return server._server.get_stats(), client._client.get_stats()


# The large-pitch pools of test_far_kernels.py: six 768 B slices into four
# 1152 B slices, entries on both sides of 2**31 and 2**32 bytes.
PITCH = 2 ** 20 + 16
SRC_POOL = Pool(0, 4101, 768, PITCH, (4100, 0, 2050, 4099, 3, 2049))
DST_POOL = Pool(16, 4101, 1152, PITCH, (4099, 0, 2051, 4100))
ND_FAR = View(0, (3, 4, 24), (2 ** 31 + 512, 2 ** 24 + 96, 2), 2)
ROWS_SRC = View(0, (5, 1040), (2 ** 30 + 4096, 1), 1)
ROWS_DST = View(0, (5, 1040), (2 ** 30 + 8192, 1), 1)


async def test_indexed_to_indexed_both_pools_far_preposted(arenas):
    case = far_case(arenas, 1, SRC_POOL, DST_POOL, "sd")
    srv, cli = await deliver(case, 61, "far indexed -> far indexed")
    assert cli["index_tx"] == 1 and srv["index_rx"] == 1
    assert srv["gpu_rx"] == 1


async def test_indexed_to_indexed_both_pools_far_send_first(arenas):
    """The descriptor, with its 64-bit stride, waits in the unexpected
    queue; a host message sent after it and received first proves that it
    has been parsed before the receive is posted."""
    case = far_case(arenas, 2, SRC_POOL, DST_POOL, "sd")
    async with loopback() as (server, client):
        sfut = client.asend(case.src_view, 62, **case.src_kw)
        marker = np.zeros(8, dtype=np.uint8)
        await client.asend(np.arange(8, dtype=np.uint8), 63)
        assert await server.arecv(marker, 63, FULL) == (63, 8)
        assert not sfut.done()
        got = await server.arecv(case.dst_view, 62, FULL, **case.dst_kw)
        await sfut
        assert got == (62, case.src.nbytes)
        case.check("far indexed -> far indexed, send first")


async def test_far_nd_source_to_contiguous(arenas):
    case = far_case(arenas, 3, ND_FAR, View.dense(0, ND_FAR.shape, 2), "s")
    assert case.src_view.stride() == (2 ** 30 + 256, 2 ** 23 + 48, 1)
    await deliver(case, 64, "far N-D -> contiguous")


async def test_contiguous_to_far_nd_window(arenas):
    case = far_case(arenas, 4, View.dense(0, ND_FAR.shape, 2), ND_FAR, "d")
    await deliver(case, 65, "contiguous -> far N-D window")


async def test_far_rows_source_to_far_rows_window(arenas):
    case = far_case(arenas, 5, ROWS_SRC, ROWS_DST, "sd")
    assert case.src_view.stride() == (2 ** 30 + 4096, 1)
    assert case.dst_view.stride() == (2 ** 30 + 8192, 1)
    await deliver(case, 66, "far rows -> far rows")


async def test_reducing_receive_far_into_its_allocation(arenas):
    """reduce="sum" float32 from a far rows source (packed into staging,
    then accumulated) into a contiguous destination that starts more than
    4 GiB + PORCH into its allocation. Integer-valued data: exact sums."""
    n = ROWS_SRC.nbytes
    dst = dense(4 * GIB + 4096 - GUARD, n)
    case = far_case(arenas, 6, ROWS_SRC, dst, "s")
    assert dst.start + PORCH > 4 * GIB + PORCH and dst.start % 4 == 0
    rng = np.random.default_rng(6)
    s = rng.integers(1, 9, n // 4).astype(np.float32)
    d = rng.integers(-8, 9, n // 4).astype(np.float32)
    case.set_message(s.view(np.uint8), d.view(np.uint8),
                     (d + s).view(np.uint8))
    acc = arenas.dst.base[dst.start:dst.start + n].view(torch.float32)
    assert acc.data_ptr() - arenas.dst.buf.data_ptr() == PORCH + 4 * GIB + 4096
    async with loopback() as (server, client):
        fut = server.arecv(acc, 67, FULL, reduce="sum")
        await client.asend(case.src_view, 67)
        await client.aflush()
        assert await fut == (67, n)
        assert server._server.get_stats()["reduce_rx"] == 1
    case.check("far rows -> reducing receive")
