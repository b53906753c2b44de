"""N-D strided device tensors through Server/Client: any torch view is a
legal send or receive buffer, the message is the bytes of t.contiguous().

Every transfer runs through tests/_guard_nd.py (numpy reference, whole
destination arena compared, source arena unchanged); byte-exact.
"""
import asyncio
import contextlib
import multiprocessing as mp

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")
import torch  # noqa: E402

import starway_amd as sw  # noqa: E402

from _guard_nd import GuardedNd, View  # noqa: E402


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


async def deliver(case: GuardedNd, tag: int, label: str):
    async with loopback() as (server, client):
        fut = server.arecv(case.dst_view, 0, 0)
        await client.asend(case.src_view, tag)
        await client.aflush()
        got_tag, length = await fut
        torch.cuda.synchronize()
        assert (got_tag, length) == (tag, case.src.nbytes)
    case.check(label)


# 24 KiB of int16: a (128, 96) matrix stored transposed, 4 spare elements
# per stored row.
TRANSPOSED = View(0, (128, 96), (2, 264), 2)
# 30 KiB of int32: logical (8, 20, 48) whose memory order is (20, 8, 48),
# rows of 48 in a pitch of 52 and a spare row per plane.
PERMUTED_3D = View(64, (8, 20, 48), (208, 9 * 208, 4), 4)
# The existing 2-D layout: 120 rows of 256 B, 320 B apart.
ROWS_2D = View(32, (120, 128), (320, 2), 2)


async def test_transposed_source_to_contiguous():
    case = GuardedNd(1, TRANSPOSED, View.dense(0, TRANSPOSED.shape, 2))
    assert not case.src_view.is_contiguous()
    await deliver(case, 21, "transposed -> contiguous")


async def test_contiguous_to_permuted_3d_window():
    case = GuardedNd(2, View.dense(0, PERMUTED_3D.shape, 4), PERMUTED_3D)
    await deliver(case, 22, "contiguous -> permuted 3-D window")


async def test_nd_source_to_2d_row_strided_destination():
    src = View(0, (96, 160), (2, 200), 2)  # transposed, 30 KiB
    case = GuardedNd(3, src, ROWS_2D)
    await deliver(case, 23, "N-D -> 2-D rows")


async def test_nd_to_nd_different_shapes():
    case = GuardedNd(4, TRANSPOSED,
                     View(16, (6, 64, 32), (2 * 34, 6 * 2 * 34 + 32, 2), 2))
    await deliver(case, 24, "N-D -> N-D")


async def test_nd_device_source_to_host_receive():
    case = GuardedNd(5, TRANSPOSED, View.dense(0, TRANSPOSED.shape, 2),
                     dst_on_host=True)
    await deliver(case, 25, "N-D device -> host")


async def test_host_send_to_nd_device_receive():
    case = GuardedNd(6, View.dense(0, PERMUTED_3D.shape, 4), PERMUTED_3D,
                     src_on_host=True)
    await deliver(case, 26, "host -> N-D device")


async def test_inbox_message_into_nd_destination():
    """256 B from a dense device tensor ride the small-message inbox; the
    N-D destination takes them through the bounce path."""
    dst = View(0, (16, 8), (2, 40), 2)
    case = GuardedNd(7, View.dense(0, dst.shape, 2), dst)
    async with loopback() as (server, client):
        await asyncio.sleep(0.3)  # inbox bring-up probe, as in test_gpu.py
        fut = server.arecv(case.dst_view, 0, 0)
        await asyncio.sleep(0.01)
        await client.asend(case.src_view, 27)
        got_tag, length = await fut
        torch.cuda.synchronize()
        assert (got_tag, length) == (27, 256)
        assert client._client.get_stats()["inbox_tx"] == 1
    case.check("inbox -> N-D")


async def test_size_mismatch_into_nd_destination_is_truncated():
    async with loopback() as (server, client):
        frame = torch.zeros(64, 100, dtype=torch.int16, device="cuda")
        window = frame[:, :96].t()  # (96, 64) view, 12 KiB
        src = torch.ones(96 * 32, dtype=torch.int16, device="cuda")  # 6 KiB
        torch.cuda.synchronize()
        fut = server.arecv(window, 0, 0)
        sfut = client.asend(src, 28)
        with pytest.raises(Exception, match="truncated"):
            await fut
        with pytest.raises(Exception, match="truncated"):
            await sfut
        torch.cuda.synchronize()
        assert frame.eq(0).all()


async def test_limits_raise_at_post_time():
    async with loopback() as (server, client):
        base = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        overlapping = base.as_strided((4, 8, 4), (2, 16, 1))
        with pytest.raises(ValueError, match="overlap"):
            server.arecv(overlapping, 0, 0)
        expanded = base[:8].expand(3, 8)
        with pytest.raises(ValueError, match="overlap"):
            server.arecv(expanded, 0, 0)
        six = torch.zeros([4] * 6, dtype=torch.uint8,
                          device="cuda")[:, :2, :2, :2, :2, :2]
        six = six.permute(5, 4, 3, 2, 1, 0)
        with pytest.raises(ValueError, match="dimensions"):
            client.asend(six, 29)
        with pytest.raises(ValueError, match="dimensions"):
            server.arecv(six, 0, 0)
        with pytest.raises(ValueError, match="dimensions"):
            client.send(six, 29, lambda: None, lambda r: None)


async def test_expanded_source_is_legal():
    src = View(0, (24, 512), (0, 2), 2)
    case = GuardedNd(8, src, View.dense(0, src.shape, 2))
    assert case.src_view.stride() == (0, 1)
    await deliver(case, 30, "expand() source")


async def test_inplace_transpose_after_first_send():
    """t_() keeps the tensor object and its data pointer but changes the
    layout; a cached interface dict keyed on the pointer alone would send
    the first message's bytes again."""
    host = np.random.default_rng(31).integers(
        -2 ** 15, 2 ** 15, (96, 128), dtype=np.int16)
    async with loopback() as (server, client):
        t = torch.from_numpy(host.copy()).cuda()
        first = torch.zeros(96 * 128, dtype=torch.int16, device="cuda")
        second = torch.zeros(96 * 128, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        fut = server.arecv(first, 0, 0)
        await client.asend(t, 31)
        await client.aflush()
        await fut
        ptr = t.data_ptr()
        t.t_()
        assert t.data_ptr() == ptr and t.shape == (128, 96)
        fut = server.arecv(second, 0, 0)
        await client.asend(t, 32)
        await client.aflush()
        await fut
        torch.cuda.synchronize()
        assert np.array_equal(first.cpu().numpy(), host.reshape(-1))
        assert np.array_equal(second.cpu().numpy(),
                              np.ascontiguousarray(host.T).reshape(-1))
        assert torch.equal(second, t.contiguous().reshape(-1))


# -- cross-process over hipIpc ------------------------------------------------

IPC_SRC = View(512, (8, 20, 48), (208, 9 * 208, 4), 4)  # 30 KiB, permuted
IPC_SEED = 9


def _nd_ipc_child(port, ready, verdict):
    import starway_amd as sw  # noqa: F811

    async def inner():
        server = sw.Server()
        server.listen("127.0.0.1", port)
        connected = asyncio.Event()
        loop = asyncio.get_running_loop()
        server.set_accept_cb(
            lambda ep: loop.call_soon_threadsafe(connected.set))
        ready.set()
        await connected.wait()
        ep = next(iter(server.list_clients()))
        case = GuardedNd(IPC_SEED, IPC_SRC,
                         View.dense(0, IPC_SRC.shape, 4))
        view = case.src_view
        # The view starts inside its allocation, not at its base.
        assert view.data_ptr() - case.src_buf.data_ptr() == IPC_SRC.start
        await server.asend(ep, view, 44)
        await server.aflush_ep(ep)
        src_now = case._fetch(case.src_buf)
        verdict.value = int(np.array_equal(src_now, case.src_host))
        await server.aclose()

    asyncio.run(inner())


async def test_cross_process_nd_ipc(port):
    """N-D source over the cross-process hipIpc path: the pull kernel packs
    the permuted view out of the remote allocation."""
    ctx = mp.get_context("spawn")
    ready = ctx.Event()
    verdict = ctx.Value("i", -1)
    p = ctx.Process(target=_nd_ipc_child, args=(port, ready, verdict))
    p.start()
    try:
        assert ready.wait(120)
        client = sw.Client()
        await client.aconnect("127.0.0.1", port)
        # Same seed as the child: the same source bytes, hence the same
        # expectation, without passing data between the processes.
        case = GuardedNd(IPC_SEED, IPC_SRC, View.dense(0, IPC_SRC.shape, 4))
        tag, ln = await client.arecv(case.dst_view, 0, 0)
        torch.cuda.synchronize()
        assert tag == 44 and ln == IPC_SRC.nbytes
        case.check("cross-process N-D")
        await client.aclose()
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            p.join()
        p.close()
    assert verdict.value == 1, "child: source arena modified or child failed"
