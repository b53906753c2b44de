"""Indexed send and receive through Server/Client: ``index=idx`` makes the
message the slices ``pool[idx]`` (a send) or scatters the message into them
(a receive), on every route an indexed buffer can take.

Every transfer runs through tests/_guard_index.py (numpy reference, whole
destination arena compared, source arena unchanged); byte-exact.
"""
import asyncio
import contextlib
import multiprocessing as mp
import os
import time
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")
import torch  # noqa: E402

import starway_amd as sw  # noqa: E402

from _guard_index import GuardedIndex, Pool, dense  # noqa: E402
from _guard_nd import View  # noqa: E402

FULL = (1 << 64) - 1


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


async def exchange(server, client, case: GuardedIndex, tag: int, label: str):
    """client -> server, receive pre-posted."""
    fut = server.arecv(case.dst_view, tag, FULL, **case.dst_kw)
    await client.asend(case.src_view, tag, **case.src_kw)
    await client.aflush()
    assert await fut == (tag, case.src.nbytes), label
    case.check(label)


async def deliver(case: GuardedIndex, tag: int, label: str):
    async with loopback() as (server, client):
        await exchange(server, client, case, tag, label)
        return server._server.get_stats(), client._client.get_stats()


def stats_of(server, client):
    return server._server.get_stats(), client._client.get_stats()


# The kernel tests' vector geometry: 11 slices of 1040 B at a 1072 B pitch.
SRC_POOL = Pool(0, 11, 1040, 1072, (7, 0, 10, 3, 3))  # repeats slice 3
DST_POOL = Pool(16, 8, 1040, 1056, (2, 7, 0, 5, 1))
N5 = 5 * 1040  # above the 4 KiB inbox / eager-inline sizes
SRC_SMALL = Pool(0, 11, 1040, 1072, (10, 0, 4))
DST_SMALL = Pool(16, 8, 1040, 1056, (7, 0, 3))
N3 = 3 * 1040  # below them


async def test_indexed_to_indexed_preposted_and_stats():
    case = GuardedIndex(1, SRC_POOL, DST_POOL)
    srv, cli = await deliver(case, 31, "indexed -> indexed, pre-posted")
    # One per message, on the side whose buffer was indexed.
    assert (cli["index_tx"], cli["index_rx"]) == (1, 0)
    assert (srv["index_tx"], srv["index_rx"]) == (0, 1)
    assert srv["gpu_rx"] == 1


async def test_indexed_to_indexed_send_first():
    """The descriptor and its index list wait in the unexpected queue. A
    host message sent after it and received first proves the indexed RTS
    frame has been parsed (and found no receive) before the receive is
    posted."""
    case = GuardedIndex(2, SRC_POOL, DST_POOL)
    async with loopback() as (server, client):
        sfut = client.asend(case.src_view, 32, **case.src_kw)
        marker = np.zeros(8, dtype=np.uint8)
        await client.asend(np.arange(8, dtype=np.uint8), 33)
        assert await server.arecv(marker, 33, FULL) == (33, 8)
        assert not sfut.done()
        tag, ln = await server.arecv(case.dst_view, 32, FULL, **case.dst_kw)
        await sfut
        assert (tag, ln) == (32, N5)
        case.check("indexed -> indexed, send first")
        srv, cli = stats_of(server, client)
        assert cli["index_tx"] == 1 and srv["index_rx"] == 1


async def test_indexed_to_indexed_slice_sizes_differ():
    src = Pool(0, 9, 768, 784, (8, 0, 4, 5, 2, 7))
    dst = Pool(16, 7, 1152, 1168, (6, 0, 3, 5))
    await deliver(GuardedIndex(3, src, dst), 34, "768 B -> 1152 B slices")


async def test_indexed_to_contiguous():
    srv, cli = await deliver(GuardedIndex(4, SRC_POOL, dense(0, N5)), 35,
                             "indexed -> contiguous")
    assert cli["index_tx"] == 1 and srv["index_rx"] == 0


async def test_contiguous_to_indexed():
    srv, cli = await deliver(GuardedIndex(5, dense(0, N5), DST_POOL), 36,
                             "contiguous -> indexed")
    assert cli["index_tx"] == 0 and srv["index_rx"] == 1


# 5200 B of int32: logical (5, 10, 26) whose memory order is (10, 5, 26),
# rows of 26 in a pitch of 28 and a spare row per plane.
WINDOW_3D = View(64, (5, 10, 26), (112, 6 * 112, 4), 4)
# 5200 B of int16: 50 rows of 104 B, 128 B apart.
ROWS_2D = View(32, (50, 52), (128, 2), 2)


async def test_indexed_to_permuted_3d_window():
    case = GuardedIndex(6, SRC_POOL, WINDOW_3D)
    assert not case.dst_view.is_contiguous()
    await deliver(case, 37, "indexed -> permuted 3-D window")


async def test_row_strided_source_to_indexed():
    case = GuardedIndex(7, ROWS_2D, DST_POOL)
    assert case.src_view.stride() == (64, 1)
    await deliver(case, 38, "2-D rows -> indexed")


async def test_indexed_source_to_numpy_receive():
    case = GuardedIndex(8, SRC_POOL, dense(0, N5), dst_on_host=True)
    await deliver(case, 39, "indexed -> host")


@pytest.mark.parametrize("src_pool,dst_pool", [(SRC_SMALL, DST_SMALL),
                                               (SRC_POOL, DST_POOL)],
                         ids=["3120B", "5200B"])
async def test_numpy_send_to_indexed_destination(src_pool, dst_pool):
    """Below and above 4 KiB: the eager frame is inline or streamed; both
    bounce and are scattered from device staging."""
    case = GuardedIndex(9, dense(0, dst_pool.nbytes), dst_pool,
                        src_on_host=True)
    srv, cli = await deliver(case, 40, "host -> indexed")
    assert srv["index_rx"] == 1 and srv["eager_rx"] + srv["gpu_rx"] >= 1


async def first_endpoint(server):
    deadline = time.monotonic() + 10
    while not server.list_clients():
        assert time.monotonic() < deadline, "no client was accepted"
        await asyncio.sleep(0.002)
    return next(iter(server.list_clients()))


async def inbox_live(server, client, ep) -> int:
    """Send small dense device messages server -> client until one rides
    the inbox (its bring-up probe has then come back). Returns the server's
    inbox_tx afterwards."""
    probe = torch.arange(64, dtype=torch.uint8, device="cuda")
    sink = torch.zeros(64, dtype=torch.uint8, device="cuda")
    deadline = time.monotonic() + 10
    while True:
        fut = client.arecv(sink, 7, FULL)
        await server.asend(ep, probe, 7)
        await fut
        sent = server._server.get_stats()["inbox_tx"]
        if sent:
            return sent
        assert time.monotonic() < deadline, "the inbox never came up"
        await asyncio.sleep(0.002)


async def test_inbox_message_into_indexed_destination():
    """3120 B from a dense device tensor ride the small-message inbox; the
    indexed destination takes them through the bounce path."""
    case = GuardedIndex(10, dense(0, N3), DST_SMALL)
    async with loopback() as (server, client):
        ep = await first_endpoint(server)
        base = await inbox_live(server, client, ep)
        fut = client.arecv(case.dst_view, 41, FULL, **case.dst_kw)
        await server.asend(ep, case.src_view, 41)
        assert await fut == (41, N3)
        srv, cli = stats_of(server, client)
        assert srv["inbox_tx"] == base + 1
        # A non-dense destination's bounce upload counts as gpu_rx, as a
        # strided one's always has.
        assert cli["index_rx"] == 1 and cli["inbox_rx"] == base
    case.check("inbox -> indexed")


async def test_small_indexed_source_stays_off_the_inbox():
    """3120 B would fit an inbox slot, but no push kernel gathers: the
    indexed source goes by rendezvous and inbox_tx does not move. A dense
    send of the same size right after it does take the inbox."""
    case = GuardedIndex(11, SRC_SMALL, dense(0, N3))
    plain = GuardedIndex(12, dense(0, N3), dense(0, N3))
    async with loopback() as (server, client):
        ep = await first_endpoint(server)
        base = await inbox_live(server, client, ep)
        gpu_rx = client._client.get_stats()["gpu_rx"]
        fut = client.arecv(case.dst_view, 42, FULL)
        await server.asend(ep, case.src_view, 42, **case.src_kw)
        assert await fut == (42, N3)
        srv, cli = stats_of(server, client)
        assert srv["inbox_tx"] == base and srv["index_tx"] == 1
        assert cli["gpu_rx"] == gpu_rx + 1 and cli["inbox_rx"] == base
        case.check("small indexed source")
        fut = client.arecv(plain.dst_view, 43, FULL)
        await server.asend(ep, plain.src_view, 43)
        assert await fut == (43, N3)
        assert server._server.get_stats()["inbox_tx"] == base + 1
        plain.check("dense send after it")


async def test_indexed_source_into_reducing_receive():
    """reduce="sum" float32 from an indexed source: gathered into staging,
    then accumulated. Integer-valued data, so the sum is exact."""
    rng = np.random.default_rng(13)
    pool_host = rng.integers(-1000, 1000, (11, 268)).astype(np.float32)
    acc_host = rng.integers(-1000, 1000, 5 * 260).astype(np.float32)
    idx = [7, 0, 10, 3, 3]
    pool = torch.from_numpy(pool_host.copy()).cuda()
    acc = torch.from_numpy(acc_host.copy()).cuda()
    torch.cuda.synchronize()
    async with loopback() as (server, client):
        fut = server.arecv(acc, 44, FULL, reduce="sum")
        await client.asend(pool[:, :260], 44, index=idx)
        await client.aflush()
        assert await fut == (44, N5)
        srv, cli = stats_of(server, client)
        assert srv["reduce_rx"] == 1 and cli["index_tx"] == 1
    torch.cuda.synchronize()
    want = acc_host + pool_host[idx, :260].reshape(-1)
    assert np.array_equal(acc.cpu().numpy(), want)
    assert np.array_equal(pool.cpu().numpy(), pool_host)


async def test_short_message_is_truncated_and_the_connection_survives():
    case = GuardedIndex(14, dense(0, N5), DST_POOL)
    short = torch.ones(N5 - 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    async with loopback() as (server, client):
        fut = server.arecv(case.dst_view, 45, FULL, **case.dst_kw)
        sfut = client.asend(short, 45)  # > 4 KiB: rendezvous
        with pytest.raises(Exception, match="truncated"):
            await fut
        with pytest.raises(Exception, match="truncated"):
            await sfut
        case.check_untouched("16 B short")
        await exchange(server, client, case, 46, "message after the refusal")


async def test_close_cancels_an_indexed_receive():
    case = GuardedIndex(15, dense(0, N5), DST_POOL)
    server = sw.Server()
    client = sw.Client()
    await client.aconnect_address(server.listen_address())
    fut = server.arecv(case.dst_view, 47, FULL, **case.dst_kw)
    await server.aflush()
    await client.aclose()
    await server.aclose()
    with pytest.raises(Exception, match="cancel"):
        await fut
    case.check_untouched("canceled")


async def test_index_list_is_copied_when_posted():
    case = GuardedIndex(16, SRC_POOL, DST_POOL)
    async with loopback() as (server, client):
        dst_idx = list(DST_POOL.index)
        src_idx = np.array(SRC_POOL.index, dtype=np.int64)
        fut = server.arecv(case.dst_view, 48, FULL, index=dst_idx)
        dst_idx[:] = [6, 6, 6, 6, 6]
        sfut = client.asend(case.src_view, 48, index=src_idx)
        src_idx[:] = 1
        await sfut
        assert await fut == (48, N5)
    case.check("lists mutated after posting")


async def test_device_only_limits_raise_at_post_time():
    async with loopback() as (server, client):
        pool = torch.zeros(8, 64, dtype=torch.int16, device="cuda")
        pool3 = torch.zeros(8, 4, 16, dtype=torch.int16, device="cuda")
        ep = await first_endpoint(server)
        posts = [
            lambda b, i, **k: client.asend(b, 49, index=i, **k),
            lambda b, i, **k: server.asend(ep, b, 49, index=i, **k),
            lambda b, i, **k: client.send(b, 49, lambda: None,
                                          lambda r: None, index=i, **k),
        ]
        recvs = [
            lambda b, i, **k: server.arecv(b, 49, FULL, index=i, **k),
            lambda b, i, **k: client.arecv(b, 49, FULL, index=i, **k),
            lambda b, i, **k: server.recv(b, 49, FULL, lambda t, n: None,
                                          lambda r: None, index=i, **k),
        ]
        for post in posts + recvs:
            with pytest.raises(ValueError, match="index limit: .*dense"):
                post(pool3[:, :, :8], [1, 2])  # a slice is not one run
            with pytest.raises(ValueError, match="index limit: .*dense"):
                post(pool.t(), [1, 2])
            with pytest.raises(ValueError, match="index limit: .*host"):
                post(pool, torch.tensor([1, 2], device="cuda"))
            with pytest.raises(ValueError, match="index limit: .*range"):
                post(pool, [8])
            with pytest.raises(ValueError, match="index limit: .*dimension"):
                post(torch.zeros((), device="cuda"), [0])
            # Empty slices: the peer would refuse the descriptor as
            # malformed and drop the connection.
            with pytest.raises(ValueError, match="index limit: .*empty"):
                post(pool[:, :0], [1, 2])
        overlapping = pool.reshape(-1).as_strided((8, 64), (32, 1))
        expanded = pool[0].expand(8, 64)
        for recv in recvs:
            with pytest.raises(ValueError, match="index limit: .*overlap"):
                recv(overlapping, [1, 2])
            with pytest.raises(ValueError, match="index limit: .*overlap"):
                recv(expanded, [1, 2])
            with pytest.raises(ValueError, match="index limit: .*repeat"):
                recv(pool, [1, 1])
            with pytest.raises(ValueError, match="index limit: .*reduce"):
                recv(pool.view(torch.float16), [1, 2], reduce="sum")
        # A source may overlap, repeat and be strided along dimension 0.
        out = torch.zeros(3 * 64, dtype=torch.int16, device="cuda")
        host = np.arange(8 * 64, dtype=np.int16).reshape(8, 64)
        pool.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        fut = server.arecv(out, 50, FULL)
        await client.asend(pool[::2], 50, index=[3, 0, 3])
        assert await fut == (50, 3 * 128)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(3, 64),
                              host[::2][[3, 0, 3]])


# -- cross-process over hipIpc ------------------------------------------------

IPC_SRC = Pool(512, 11, 1040, 1072, (7, 0, 10, 3, 3))
IPC_SEED = 17


def _index_ipc_child(port, ready, verdict):
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
        case = GuardedIndex(IPC_SEED, IPC_SRC, DST_POOL)
        view = case.src_view
        # The pool starts inside its allocation, not at its base.
        assert view.data_ptr() - case.src_buf.data_ptr() == IPC_SRC.start
        await server.asend(ep, view, 51, **case.src_kw)
        await server.aflush_ep(ep)
        src_now = case._fetch(case.src_buf)
        verdict.value = int(np.array_equal(src_now, case.src_host))
        await server.aclose()

    asyncio.run(inner())


async def test_cross_process_indexed_ipc(port):
    """Indexed source over the cross-process hipIpc path: the pool is read
    through the mapping, the index list arrives in the frame."""
    ctx = mp.get_context("spawn")
    ready = ctx.Event()
    verdict = ctx.Value("i", -1)
    p = ctx.Process(target=_index_ipc_child, args=(port, ready, verdict))
    p.start()
    try:
        assert ready.wait(120)
        client = sw.Client()
        await client.aconnect("127.0.0.1", port)
        # Same seed as the child: the same source bytes, hence the same
        # expectation, without passing data between the processes.
        case = GuardedIndex(IPC_SEED, IPC_SRC, DST_POOL)
        tag, ln = await client.arecv(case.dst_view, 0, 0, **case.dst_kw)
        assert tag == 51 and ln == N5
        case.check("cross-process indexed")
        assert client._client.get_stats()["index_rx"] == 1
        await client.aclose()
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            p.join()
        p.close()
    assert verdict.value == 1, "child: source arena modified or child failed"


# -- cross-host route ---------------------------------------------------------

async def _xhost_body():
    """Every device send is downloaded to host staging and shipped eagerly:
    the indexed source is gathered into device staging first, and the
    indexed destination is scattered from device staging."""
    case = GuardedIndex(18, SRC_POOL, DST_POOL)
    async with loopback() as (server, client):
        await exchange(server, client, case, 52, "cross-host route")
        srv, cli = stats_of(server, client)
        assert srv["eager_rx"] + srv["gpu_rx"] == 1 and srv["cma_rx"] == 0
        assert cli["index_tx"] == 1 and srv["index_rx"] == 1
        assert cli["inbox_tx"] == 0


def _child(q):
    try:
        assert os.environ.get("STARWAY_FORCE_XHOST") == "1"
        asyncio.run(asyncio.wait_for(_xhost_body(), timeout=120))
        q.put("ok")
    except BaseException:  # noqa: BLE001 - the parent reports it
        q.put(traceback.format_exc())


def test_cross_host_route_in_a_child():
    """STARWAY_FORCE_XHOST is read once per process: a fresh child, started
    with the variable already in its environment."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(q,))
    before = os.environ.get("STARWAY_FORCE_XHOST")
    os.environ["STARWAY_FORCE_XHOST"] = "1"
    try:
        p.start()
    finally:
        if before is None:
            del os.environ["STARWAY_FORCE_XHOST"]
        else:
            os.environ["STARWAY_FORCE_XHOST"] = before
    try:
        assert q.get(timeout=180) == "ok"
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            p.join()
        p.close()
