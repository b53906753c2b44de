"""Reducing receive (``arecv(..., reduce="sum")``) through the engine, on
every plane that can deliver one, bit-exact.

The destination is always a slice of a larger device arena, so the bytes
around it are part of the verdict, and every sender's buffer is checked
unchanged. Inputs, the torch-on-CPU expectation and the arena checks:
tests/_guard_accum.py.

Ordering is made deterministic without sleeping: a completed ``aflush()`` on
the receiver proves every receive issued before it is posted (an engine
processes its commands in order), and a delivered host sentinel proves every
earlier message on that connection has been parsed (one connection is one
ordered stream).
"""
import asyncio
import contextlib
import multiprocessing as mp
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import starway_amd as sw  # noqa: E402

from _guard_accum import GuardedAccum, itemsize  # noqa: E402

FULL = (1 << 64) - 1
DTYPE_NAMES = ["float32", "float16", "bfloat16", "int32"]
SENTINEL = 0xFEED
NP_DTYPES = {"float32": np.float32, "float16": np.float16,
             "bfloat16": np.uint16, "int32": np.int32}


@contextlib.asynccontextmanager
async def loopback(n_clients=1):
    server = sw.Server()
    clients = [sw.Client() for _ in range(n_clients)]
    addr = server.listen_address()
    for c in clients:
        await c.aconnect_address(addr)
    try:
        if n_clients == 1:
            yield server, clients[0]
        else:
            yield server, clients
    finally:
        for c in clients:
            await c.aclose()
        await server.aclose()


def stats(end):
    return (end._server if hasattr(end, "_server") else end._client).get_stats()


def delta(after, before, *keys):
    return {k: after[k] - before[k] for k in keys}


async def parsed_up_to_here(server, client):
    """Returns once the server has parsed everything `client` sent so far."""
    flag = np.zeros(1, dtype=np.uint8)
    fut = server.arecv(flag, SENTINEL, FULL)
    await client.asend(np.ones(1, dtype=np.uint8), SENTINEL)
    await fut


async def inbox_ready(server, client):
    """Plain small device messages until one rides the inbox plane (its
    bring-up probe completes a little after connect)."""
    src = torch.arange(16, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(5000):
        before = stats(client)["inbox_tx"]
        fut = server.arecv(dst, SENTINEL + 1, FULL)
        await client.asend(src, SENTINEL + 1)
        await fut
        if stats(client)["inbox_tx"] > before:
            return
    raise AssertionError("the inbox plane never came up")


async def plain_message_still_delivered(server, client, tag=77):
    """The connection survived: a following plain message arrives."""
    src = torch.arange(300, dtype=torch.int32, device="cuda")
    dst = torch.zeros(300, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fut = server.arecv(dst, tag, FULL)
    await client.asend(src, tag)
    assert tuple(await fut) == (tag, 1200)
    torch.cuda.synchronize()
    assert torch.equal(src, dst)


# -- rendezvous ---------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
async def test_rendezvous_preposted(dtype):
    es = itemsize(dtype)
    case = GuardedAccum(100, dtype, (1 << 20) + 3 * es)
    async with loopback() as (server, client):
        before = stats(server)
        fut = server.arecv(case.dst_view, 7, FULL, reduce="sum")
        await server.aflush()
        await client.asend(case.src_view, 7)
        assert tuple(await fut) == (7, case.nbytes)
        case.check(f"pre-posted rendezvous {dtype}")
        assert delta(stats(server), before, "reduce_rx", "gpu_rx",
                     "msgs_received") == {
            "reduce_rx": 1, "gpu_rx": 1, "msgs_received": 1}


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
async def test_rendezvous_unexpected(dtype):
    es = itemsize(dtype)
    case = GuardedAccum(110, dtype, (128 << 10) + 3 * es, src_off=es,
                        dst_off=es)
    async with loopback() as (server, client):
        before = stats(server)
        send = client.asend(case.src_view, 8)
        await parsed_up_to_here(server, client)
        case.check_untouched("before the receive is posted")
        assert tuple(await server.arecv(case.dst_view, 8, FULL,
                                        reduce="sum")) == (8, case.nbytes)
        await send
        case.check(f"unexpected rendezvous {dtype}")
        assert delta(stats(server), before, "reduce_rx")["reduce_rx"] == 1


async def test_batching_window_never_overwrites():
    """Eight batch-sized messages into ONE accumulator, all receives posted
    first. k_copy_multi would overwrite; small-integer values make the sum
    independent of the order the contributions land in."""
    nbytes = (8 << 10) + 4
    case = GuardedAccum(120, "float32", nbytes, small_ints=True)
    rng = np.random.default_rng(121)
    hosts = [case.src_words.view(np.float32).copy()] + [
        rng.integers(1, 8, nbytes // 4).astype(np.float32) for _ in range(7)]
    srcs = [torch.from_numpy(h.copy()).cuda() for h in hosts]
    torch.cuda.synchronize()
    acc = torch.from_numpy(case.dst_words.view(np.float32).copy())
    for h in hosts:
        acc = acc + torch.from_numpy(h)
    expected = case.dst_host.copy()
    d0 = case.dst.start
    expected[d0:d0 + nbytes] = acc.numpy().view(np.uint8)
    async with loopback() as (server, client):
        before = stats(server)
        futs = [server.arecv(case.dst_view, tag, FULL, reduce="sum")
                for tag in range(8)]
        await server.aflush()
        await asyncio.gather(*[client.asend(srcs[tag], tag)
                               for tag in range(8)])
        for tag, fut in enumerate(futs):
            assert tuple(await fut) == (tag, nbytes)
        case.check_against(expected, "eight contributions")
        for h, s in zip(hosts, srcs):
            assert np.array_equal(s.cpu().numpy(), h), "sender buffer changed"
        assert delta(stats(server), before, "reduce_rx")["reduce_rx"] == 8


# -- inbox plane ----------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
async def test_inbox_plane(dtype):
    """Never handed to the unpack kernel as a direct destination (it
    overwrites): the pinned bounce, then an accumulate."""
    async with loopback() as (server, client):
        await inbox_ready(server, client)
        for k, nbytes in enumerate([64, 4096]):
            pre = GuardedAccum(130 + k, dtype, nbytes, dst_off=16)
            before = stats(server)
            fut = server.arecv(pre.dst_view, 1, FULL, reduce="sum")
            await server.aflush()
            await client.asend(pre.src_view, 1)
            assert tuple(await fut) == (1, nbytes)
            pre.check(f"pre-posted inbox {nbytes} B {dtype}")
            assert delta(stats(server), before, "inbox_rx", "doorbell_rx",
                         "reduce_rx") == {
                "inbox_rx": 1, "doorbell_rx": 0, "reduce_rx": 1}

            late = GuardedAccum(140 + k, dtype, nbytes, src_off=16)
            before = stats(server)
            await client.asend(late.src_view, 2)
            await parsed_up_to_here(server, client)
            late.check_untouched("before the receive is posted")
            assert tuple(await server.arecv(late.dst_view, 2, FULL,
                                            reduce="sum")) == (2, nbytes)
            late.check(f"unexpected inbox {nbytes} B {dtype}")
            assert delta(stats(server), before, "inbox_rx", "doorbell_rx",
                         "reduce_rx") == {
                "inbox_rx": 1, "doorbell_rx": 0, "reduce_rx": 1}


async def _doorbell_scenario():
    """With the doorbell on, a lone posted small device recv is what gets
    armed. A reducing one never is: the wait kernel overwrites."""
    from _guard import GuardedCopy, Region

    async with loopback() as (server, client):
        await inbox_ready(server, client)
        ep = next(iter(server.list_clients()))

        def rung():
            return stats(server)["doorbell_rx"] + stats(client)["doorbell_rx"]

        # Pre-posted PLAIN ping-pong first, the traffic of
        # tests/test_gpu_doorbell.py: these receives are what the doorbell
        # arms for. Whether it also DELIVERS one is a matter of timing and
        # was rare where this was written (one ring in 200 round trips in
        # one run, none in another), so the count is reported, not
        # asserted: an assertion here would fail at random. What is
        # asserted is below: with the same switch on and the same traffic,
        # no reducing receive is ever delivered by a doorbell.
        for it in range(48):
            ping = GuardedCopy(7_000 + it, Region.flat(it % 2, 256),
                               Region.flat(0, 256))
            pong = GuardedCopy(7_500 + it, Region.flat(0, 256),
                               Region.flat(3, 256))
            sfut = server.arecv(ping.dst_view, 4, FULL)
            await asyncio.sleep(0)
            await client.asend(ping.src_view, 4)
            assert tuple(await sfut) == (4, 256)
            cfut = client.arecv(pong.dst_view, 5, FULL)
            await asyncio.sleep(0)
            await server.asend(ep, pong.src_view, 5)
            assert tuple(await cfut) == (5, 256)
            ping.check(f"plain ping {it}")
            pong.check(f"plain pong {it}")
        rang = rung()
        # Now the same traffic with reducing receives, on both engines.
        before = stats(server), stats(client)
        for it in range(6):
            ping = GuardedAccum(150 + it, "float32", 256 + 4 * it, dst_off=4)
            pong = GuardedAccum(160 + it, "bfloat16", 256 + 4 * it)
            sfut = server.arecv(ping.dst_view, 3, FULL, reduce="sum")
            await server.aflush()
            await asyncio.sleep(0)
            await client.asend(ping.src_view, 3)
            assert tuple(await sfut) == (3, ping.nbytes)
            cfut = client.arecv(pong.dst_view, 6, FULL, reduce="sum")
            await client.aflush()
            await asyncio.sleep(0)
            await server.asend(ep, pong.src_view, 6)
            assert tuple(await cfut) == (6, pong.nbytes)
            ping.check(f"doorbell on, reducing ping {it}")
            pong.check(f"doorbell on, reducing pong {it}")
        for end, b in zip((server, client), before):
            d = delta(stats(end), b, "inbox_rx", "doorbell_rx", "reduce_rx")
            assert d == {"inbox_rx": 6, "doorbell_rx": 0, "reduce_rx": 6}, d
        return {"doorbell_rx_plain": rang}


def _doorbell_child(q):
    import os

    os.environ["STARWAY_DOORBELL"] = "1"  # opt-in; read at first use
    try:
        info = asyncio.run(asyncio.wait_for(_doorbell_scenario(), timeout=60))
        q.put(("ok", info))
    except BaseException:
        q.put(("failed", traceback.format_exc()))


def test_doorbell_never_arms_a_reducing_recv():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_doorbell_child, args=(q,))
    p.start()
    try:
        state, info = q.get(timeout=180)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            p.join()
        p.close()
    assert state == "ok", info
    print(info)


# -- host sender ----------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
async def test_host_sender(dtype):
    """Every bounce ends in begin_h2d: staging, then accumulate."""
    npdt = NP_DTYPES[dtype]
    async with loopback() as (server, client):
        for k, nbytes in enumerate([64, 64 << 10, 2 << 20]):
            case = GuardedAccum(160 + k, dtype, nbytes, dst_off=16,
                                src_on_host=True)
            before = stats(server)
            fut = server.arecv(case.dst_view, 5, FULL, reduce="sum")
            await server.aflush()
            await client.asend(case.src_view.view(npdt), 5)
            assert tuple(await fut) == (5, nbytes)
            case.check(f"host sender {nbytes} B {dtype}")
            assert delta(stats(server), before, "reduce_rx")["reduce_rx"] == 1
        case = GuardedAccum(170, dtype, 64 << 10, src_on_host=True)
        await client.asend(case.src_view.view(npdt), 6)
        await parsed_up_to_here(server, client)
        case.check_untouched("before the receive is posted")
        assert tuple(await server.arecv(case.dst_view, 6, FULL,
                                        reduce="sum")) == (6, 64 << 10)
        case.check(f"unexpected host sender {dtype}")


# -- sources the fast route cannot read in place ----------------------------------


async def test_strided_sources():
    """A transposed matrix (N-D) and a row-strided slice into a contiguous
    reducing receive: packed into staging, then accumulated. The result is
    the initial values plus src.contiguous()."""
    rows, cols = 67, 129
    async with loopback() as (server, client):
        for k, kind in enumerate(["transposed", "rows"]):
            case = GuardedAccum(180 + k, "float32", rows * cols * 4,
                                dst_off=4 * k)
            msg = case.src_words.view(np.int32).reshape(rows, cols)
            if kind == "transposed":
                host = np.ascontiguousarray(msg.T)
                base = torch.from_numpy(host.copy()).cuda().view(torch.float32)
                view = base.t()
            else:
                host = np.zeros((rows, cols + 31), dtype=np.int32)
                host[:, :cols] = msg
                base = torch.from_numpy(host.copy()).cuda().view(torch.float32)
                view = base[:, :cols]
            assert not view.is_contiguous() and view.shape == (rows, cols)
            torch.cuda.synchronize()
            fut = server.arecv(case.dst_view, 9, FULL, reduce="sum")
            await server.aflush()
            await client.asend(view, 9)
            assert tuple(await fut) == (9, case.nbytes)
            case.check_against(case.expected, f"{kind} source")
            assert np.array_equal(
                base.view(torch.int32).cpu().numpy(), host), "source changed"


async def test_element_misaligned_source():
    """fp32 data behind a uint8 view at byte offset 1."""
    nbytes = 4 * 4097
    case = GuardedAccum(190, "float32", nbytes)
    raw = np.zeros(nbytes + 16, dtype=np.uint8)
    raw[1:1 + nbytes] = case.src_words.view(np.uint8)
    dev = torch.from_numpy(raw.copy()).cuda()
    view = dev[1:1 + nbytes]
    assert view.data_ptr() % 4 == 1
    torch.cuda.synchronize()
    async with loopback() as (server, client):
        fut = server.arecv(case.dst_view, 10, FULL, reduce="sum")
        await server.aflush()
        await client.asend(view, 10)
        assert tuple(await fut) == (10, nbytes)
        case.check_against(case.expected, "misaligned source")
        assert np.array_equal(dev.cpu().numpy(), raw), "source changed"


# -- prefix, zero length ----------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
async def test_prefix_and_zero_length(dtype):
    es = itemsize(dtype)
    nbytes = (64 << 10) + es
    case = GuardedAccum(200, dtype, nbytes, dst_cap=2 * nbytes)
    async with loopback() as (server, client):
        assert case.dst_view.numel() * es == 2 * nbytes
        fut = server.arecv(case.dst_view, 11, FULL, reduce="sum")
        await server.aflush()
        await client.asend(case.src_view, 11)
        assert tuple(await fut) == (11, nbytes)
        case.check(f"prefix {dtype}")  # the second half is unchanged
        fut = server.arecv(case.dst_view, 12, FULL, reduce="sum")
        await server.aflush()
        await client.asend(np.zeros(0, dtype=np.uint8), 12)
        assert tuple(await fut) == (12, 0)
        case.check(f"after a zero-length message {dtype}")


# -- failures ---------------------------------------------------------------------


async def test_length_not_a_multiple_of_the_item_size():
    async with loopback() as (server, client):
        await inbox_ready(server, client)
        # Rendezvous size: both sides fail.
        case = GuardedAccum(210, "float32", 256 << 10)
        odd = torch.ones((128 << 10) + 2, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fut = server.arecv(case.dst_view, 13, FULL, reduce="sum")
        await server.aflush()
        send = client.asend(odd, 13)
        with pytest.raises(Exception, match="reduce"):
            await fut
        with pytest.raises(Exception, match="reduce"):
            await send
        case.check_untouched("rendezvous, odd length")
        await plain_message_still_delivered(server, client)
        # Inbox size: only the receiver fails.
        case = GuardedAccum(211, "float32", 256)
        before = stats(client)["inbox_tx"]
        fut = server.arecv(case.dst_view, 14, FULL, reduce="sum")
        await server.aflush()
        await client.asend(odd[:62], 14)
        assert stats(client)["inbox_tx"] == before + 1
        with pytest.raises(Exception, match="reduce"):
            await fut
        case.check_untouched("inbox, odd length")
        await plain_message_still_delivered(server, client)
        # Host sender (eager): only the receiver fails.
        case = GuardedAccum(212, "float16", 256)
        fut = server.arecv(case.dst_view, 15, FULL, reduce="sum")
        await server.aflush()
        await client.asend(np.ones(33, dtype=np.uint8), 15)
        with pytest.raises(Exception, match="reduce"):
            await fut
        case.check_untouched("eager, odd length")
        await plain_message_still_delivered(server, client)
        assert stats(server)["reduce_rx"] == 0


async def test_longer_than_the_buffer_is_truncated():
    async with loopback() as (server, client):
        case = GuardedAccum(220, "float32", 64 << 10)
        big = torch.ones(128 << 10, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fut = server.arecv(case.dst_view, 16, FULL, reduce="sum")
        await server.aflush()
        send = client.asend(big, 16)
        with pytest.raises(Exception, match="truncated"):
            await fut
        with pytest.raises(Exception, match="truncated"):
            await send
        case.check_untouched("too long")
        await plain_message_still_delivered(server, client)


async def test_cancel_leaves_the_buffer_untouched():
    case = GuardedAccum(230, "bfloat16", 4096)
    server = sw.Server()
    client = sw.Client()
    await client.aconnect_address(server.listen_address())
    fut = server.arecv(case.dst_view, 17, FULL, reduce="sum")
    await server.aflush()
    await client.aclose()
    await server.aclose()
    with pytest.raises(Exception, match="cancel"):
        await fut
    case.check_untouched("canceled")


async def test_posting_limits_on_device_buffers():
    """Refused when the receive is posted; the error names the limit."""
    async with loopback() as (server, client):
        for end in (server, client):
            for dt in (torch.uint8, torch.float64, torch.int64):
                buf = torch.zeros(64, dtype=dt, device="cuda")
                with pytest.raises(ValueError, match="dtype"):
                    end.arecv(buf, 0, 0, reduce="sum")
            big = torch.zeros(16, 32, dtype=torch.float32, device="cuda")
            with pytest.raises(ValueError, match="contiguous"):
                end.arecv(big[:, :8], 0, 0, reduce="sum")   # 2-D row-strided
            with pytest.raises(ValueError, match="contiguous"):
                end.arecv(big.t(), 0, 0, reduce="sum")      # N-D
            raw = torch.zeros(64, dtype=torch.uint8, device="cuda")
            native = end._server if end is server else end._client
            shim = sw._norm_buffer(raw[1:33])  # fp32 data at an odd address
            with pytest.raises(ValueError, match="aligned"):
                native.recv(shim, 0, 0, None, None, reduce="sum",
                            dtype="float32")
            with pytest.raises(ValueError, match="max"):
                end.arecv(big, 0, 0, reduce="max")
        torch.cuda.synchronize()
        assert not big.any() and not raw.any()


# -- fan-in -----------------------------------------------------------------------


async def test_fan_in_four_clients():
    """Four clients x 8 messages into one accumulator through 32 wildcard
    reducing receives posted up front. One message rides the inbox plane,
    the rest the rendezvous plane (batch-sized and larger); a message
    shorter than the buffer adds into the prefix."""
    n = (128 << 10) // 4 + 1  # elements of the accumulator
    case = GuardedAccum(240, "float32", 4 * n, small_ints=True)
    rng = np.random.default_rng(241)
    sizes = [n, (8 << 10) // 4 + 1, n, 2049, (8 << 10) // 4 + 1, n, 1500, n]
    hosts, devs = [], []
    for c in range(4):
        for m in range(8):
            count = 256 if (c, m) == (0, 0) else sizes[m]  # 1 KiB: inbox
            h = rng.integers(1, 8, count).astype(np.float32)
            hosts.append(h)
            devs.append(torch.from_numpy(h.copy()).cuda())
    torch.cuda.synchronize()
    acc = torch.from_numpy(case.dst_words.view(np.float32).copy())
    for h in hosts:
        acc[:h.size] += torch.from_numpy(h)
    expected = case.dst_host.copy()
    d0 = case.dst.start
    expected[d0:d0 + 4 * n] = acc.numpy().view(np.uint8)
    async with loopback(4) as (server, clients):
        await inbox_ready(server, clients[0])
        before = stats(server)
        futs = [server.arecv(case.dst_view, 0, 0, reduce="sum")
                for _ in range(32)]
        await server.aflush()
        sends = [clients[c].asend(devs[8 * c + m], 1000 + 8 * c + m)
                 for m in range(8) for c in range(4)]
        await asyncio.gather(*sends)
        got = [tuple(await f) for f in futs]
        assert sorted(t for t, _ in got) == list(range(1000, 1032))
        lens = {t: ln for t, ln in got}
        for i, h in enumerate(hosts):
            assert lens[1000 + i] == 4 * h.size
        case.check_against(expected, "fan-in")
        for h, d in zip(hosts, devs):
            assert np.array_equal(d.cpu().numpy(), h), "sender buffer changed"
        d = delta(stats(server), before, "reduce_rx", "inbox_rx")
        assert d == {"reduce_rx": 32, "inbox_rx": 1}, d


# -- cross-process over hipIpc ---------------------------------------------------------

IPC_DEV_BYTES = (256 << 10) + 12
IPC_HOST_BYTES = (1 << 20) + 12


def _ipc_cases():
    out = []
    for k, dtype in enumerate(DTYPE_NAMES):
        out.append((GuardedAccum(300 + k, dtype, IPC_DEV_BYTES, src_off=16),
                    GuardedAccum(310 + k, dtype, IPC_HOST_BYTES,
                                 src_on_host=True)))
    return out


def _ipc_child(port, ready, verdict):
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
        cases = _ipc_cases()
        for k, (dev, host) in enumerate(cases):
            await server.asend(ep, dev.src_view, 2 * k)
            await server.asend(ep, host.src_view, 2 * k + 1)
        await server.aflush_ep(ep)
        ok = True
        for dev, host in cases:
            try:
                dev.check_source("child")
                host.check_source("child")
            except AssertionError:
                ok = False
        verdict.value = int(ok)
        await server.aclose()

    asyncio.run(inner())


async def test_cross_process_ipc_and_cma(port):
    """The child sends; per dtype one contiguous device message (the
    accumulate kernel reads the hipIpc mapping in place) and one host array
    of 1 MiB + 12 (CMA pull, or its eager fallback, into a bounce)."""
    ctx = mp.get_context("spawn")
    ready = ctx.Event()
    verdict = ctx.Value("i", -1)
    p = ctx.Process(target=_ipc_child, args=(port, ready, verdict))
    p.start()
    try:
        assert ready.wait(120)
        client = sw.Client()
        await client.aconnect("127.0.0.1", port)
        # Same seeds as the child: the same source bytes, hence the same
        # expectation, without passing data between the processes.
        cases = _ipc_cases()
        futs = []
        for k, (dev, host) in enumerate(cases):
            futs.append(client.arecv(dev.dst_view, 2 * k, FULL, reduce="sum"))
            futs.append(client.arecv(host.dst_view, 2 * k + 1, FULL,
                                     reduce="sum"))
        for k, (dev, host) in enumerate(cases):
            assert tuple(await futs[2 * k]) == (2 * k, IPC_DEV_BYTES)
            assert tuple(await futs[2 * k + 1]) == (2 * k + 1, IPC_HOST_BYTES)
        for dev, host in cases:
            dev.check_against(dev.expected, f"hipIpc {dev.dtype}")
            host.check_against(host.expected, f"CMA {host.dtype}")
        assert stats(client)["reduce_rx"] == 8
        await client.aclose()
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            p.join()
        p.close()
    assert verdict.value == 1, "child: a source arena changed or child failed"


# -- two devices --------------------------------------------------------------------


@pytest.mark.skipif(sw.gpu_device_count() < 2, reason="needs two GPUs")
async def test_two_source_devices_one_accumulator():
    """Sources on devices 0 and 1, all summed into one accumulator on device
    0, every receive posted at once. Plain pulls would ride two lanes (one
    per source device) and run concurrently; two read-modify-write kernels
    on one buffer must not, so reducing pulls share lane 0."""
    n = (1 << 20) // 4 + 1
    torch.cuda.set_device(0)
    case = GuardedAccum(400, "float32", 4 * n, small_ints=True)
    rng = np.random.default_rng(401)
    hosts = [rng.integers(1, 8, n).astype(np.float32) for _ in range(8)]
    devs = [torch.from_numpy(h.copy()).to(f"cuda:{i % 2}")
            for i, h in enumerate(hosts)]
    torch.cuda.synchronize(0)
    torch.cuda.synchronize(1)
    acc = torch.from_numpy(case.dst_words.view(np.float32).copy())
    for h in hosts:
        acc += torch.from_numpy(h)
    expected = case.dst_host.copy()
    d0 = case.dst.start
    expected[d0:d0 + 4 * n] = acc.numpy().view(np.uint8)
    async with loopback() as (server, client):
        futs = [server.arecv(case.dst_view, i, FULL, reduce="sum")
                for i in range(8)]
        await server.aflush()
        await asyncio.gather(*[client.asend(devs[i], i) for i in range(8)])
        for i, fut in enumerate(futs):
            assert tuple(await fut) == (i, 4 * n)
        case.check_against(expected, "two source devices")
        for h, d in zip(hosts, devs):
            assert np.array_equal(d.cpu().numpy(), h), "sender buffer changed"
