"""Converting receive (``arecv(..., msg_dtype=...)``) through the engine, on
every plane that can deliver one, bit-exact against torch on the CPU.

The destination is always a slice of a larger device arena, so the bytes
around it are part of the verdict, and every sender's buffer is checked
unchanged. Inputs, the expectation and the arena checks:
tests/_guard_cast.py.

Ordering is made deterministic without sleeping, as in
tests/test_gpu_reduce.py: a completed ``aflush()`` on the receiver proves
every receive issued before it is posted, and a delivered host sentinel
proves every earlier message on that connection has been parsed.
"""
import asyncio
import contextlib
import multiprocessing as mp

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import starway_amd as sw  # noqa: E402

from _guard_cast import GuardedCast, itemsize  # noqa: E402

FULL = (1 << 64) - 1
SENTINEL = 0xFEED
# (destination, message): one narrowing and one widening pair.
NARROW = ("bfloat16", "float32")
WIDEN = ("float32", "bfloat16")
MODES = [pytest.param(*NARROW, False, id="f32-to-bf16"),
         pytest.param(*NARROW, True, id="f32-to-bf16-sum"),
         pytest.param(*WIDEN, False, id="bf16-to-f32"),
         pytest.param(*WIDEN, True, id="bf16-to-f32-sum")]
modes = pytest.mark.parametrize("dst,src,acc", MODES)


@contextlib.asynccontextmanager
async def loopback():
    server = sw.Server()
    client = sw.Client()
    await client.aconnect_address(server.listen_address())
    try:
        yield server, client
    finally:
        await client.aclose()
        await server.aclose()


def stats(end):
    return (end._server if hasattr(end, "_server") else end._client).get_stats()


def delta(after, before, *keys):
    return {k: after[k] - before[k] for k in keys}


def post(end, case, tag):
    """The converting receive of `case`, reducing when the case accumulates."""
    return end.arecv(case.dst_view, tag, FULL, msg_dtype=case.src_dtype,
                     reduce="sum" if case.accumulate else None)


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


@modes
async def test_rendezvous_preposted(dst, src, acc):
    n = (1 << 20) // itemsize(src) + 3
    case = GuardedCast(600, dst, src, n, accumulate=acc)
    async with loopback() as (server, client):
        before = stats(server)
        fut = post(server, case, 7)
        await server.aflush()
        await client.asend(case.src_view, 7)
        assert tuple(await fut) == (7, case.nbytes)
        case.check("pre-posted rendezvous")
        assert delta(stats(server), before, "cast_rx", "reduce_rx", "gpu_rx",
                     "msgs_received") == {
            "cast_rx": 1, "reduce_rx": int(acc), "gpu_rx": 1,
            "msgs_received": 1}


@modes
async def test_rendezvous_unexpected(dst, src, acc):
    n = (1 << 20) // itemsize(src) + 3
    case = GuardedCast(610, dst, src, n, accumulate=acc,
                       src_off=itemsize(src), dst_off=itemsize(dst))
    async with loopback() as (server, client):
        before = stats(server)
        send = client.asend(case.src_view, 8)
        await parsed_up_to_here(server, client)
        case.check_untouched("before the receive is posted")
        assert tuple(await post(server, case, 8)) == (8, case.nbytes)
        await send
        case.check("unexpected rendezvous")
        assert delta(stats(server), before, "cast_rx", "reduce_rx") == {
            "cast_rx": 1, "reduce_rx": int(acc)}


# -- inbox plane ----------------------------------------------------------------


@modes
async def test_inbox_size_message_converts(dst, src, acc):
    """1 KiB rides the inbox plane. It must convert, not land raw: never
    handed to the unpack kernel as a direct destination."""
    n = 1024 // itemsize(src)
    async with loopback() as (server, client):
        await inbox_ready(server, client)
        pre = GuardedCast(620, dst, src, n, accumulate=acc, dst_off=16)
        before = stats(server)
        sent = stats(client)["inbox_tx"]
        fut = post(server, pre, 1)
        await server.aflush()
        await client.asend(pre.src_view, 1)
        assert tuple(await fut) == (1, 1024)
        assert stats(client)["inbox_tx"] == sent + 1
        pre.check("pre-posted inbox")
        assert delta(stats(server), before, "inbox_rx", "doorbell_rx",
                     "cast_rx", "reduce_rx") == {
            "inbox_rx": 1, "doorbell_rx": 0, "cast_rx": 1,
            "reduce_rx": int(acc)}
        late = GuardedCast(621, dst, src, n, accumulate=acc, src_off=16)
        before = stats(server)
        await client.asend(late.src_view, 2)
        await parsed_up_to_here(server, client)
        late.check_untouched("before the receive is posted")
        assert tuple(await post(server, late, 2)) == (2, 1024)
        late.check("unexpected inbox")
        assert delta(stats(server), before, "inbox_rx", "cast_rx") == {
            "inbox_rx": 1, "cast_rx": 1}


# -- the batching window, and what the feature is for -----------------------------


async def test_eight_bf16_ones_into_an_fp32_accumulator_at_256():
    """Eight batch-sized (8 KiB) bf16 messages of 1.0 into ONE accumulator
    holding 256.0, all eight receives posted first. In fp32 the result is
    264.0 everywhere. A bf16 accumulator under the existing reduce="sum"
    rounds after every contribution and stays at 256.0."""
    n = (8 << 10) // 2
    guard = 64
    ones = [torch.ones(n, dtype=torch.bfloat16, device="cuda")
            for _ in range(8)]
    arena32 = torch.full((guard + n + guard,), 256.0, dtype=torch.float32,
                         device="cuda")
    arena16 = torch.full((guard + n + guard,), 256.0, dtype=torch.bfloat16,
                         device="cuda")
    acc32 = arena32[guard:guard + n]
    acc16 = arena16[guard:guard + n]
    torch.cuda.synchronize()
    async with loopback() as (server, client):
        before = stats(server)
        futs = [server.arecv(acc32, tag, FULL, reduce="sum",
                             msg_dtype=torch.bfloat16) for tag in range(8)]
        futs += [server.arecv(acc16, 8 + tag, FULL, reduce="sum")
                 for tag in range(8)]
        await server.aflush()
        await asyncio.gather(*[client.asend(ones[tag % 8], tag)
                               for tag in range(16)])
        for tag, fut in enumerate(futs):
            assert tuple(await fut) == (tag, 2 * n)
        torch.cuda.synchronize()
        assert delta(stats(server), before, "cast_rx", "reduce_rx") == {
            "cast_rx": 8, "reduce_rx": 16}
    got32, got16 = arena32.cpu(), arena16.cpu()
    assert (got32[guard:guard + n] == 264.0).all()
    assert (got16[guard:guard + n].float() == 256.0).all()
    assert not torch.equal(got32[guard:guard + n],
                           got16[guard:guard + n].float())
    for arena in (got32, got16):
        assert (arena[:guard] == 256.0).all() and \
            (arena[guard + n:] == 256.0).all(), "guard band changed"
    for t in ones:
        assert (t.cpu().float() == 1.0).all(), "sender buffer changed"


# -- other senders ----------------------------------------------------------------


@modes
async def test_host_sender(dst, src, acc):
    """Every bounce ends in begin_h2d: staging, then the convert kernel."""
    async with loopback() as (server, client):
        for k, n in enumerate([32, (64 << 10) // itemsize(src) + 1]):
            case = GuardedCast(640 + k, dst, src, n, accumulate=acc,
                               dst_off=16, src_on_host=True)
            before = stats(server)
            fut = post(server, case, 5)
            await server.aflush()
            await client.asend(case.src_view, 5)
            assert tuple(await fut) == (5, case.nbytes)
            case.check(f"host sender n={n}")
            assert delta(stats(server), before, "cast_rx")["cast_rx"] == 1


@modes
async def test_rows_sender(dst, src, acc):
    """t[:, :half] of a 2-D device tensor: packed into staging, then
    converted. The message is t[:, :half].contiguous()."""
    rows, half = 67, 129
    case = GuardedCast(650, dst, src, rows * half, accumulate=acc)
    words = case.src_words.reshape(rows, half)
    host = np.zeros((rows, 2 * half), dtype=words.dtype)
    host[:, :half] = words
    signed = {2: np.int16, 4: np.int32}[words.itemsize]
    base = torch.from_numpy(host.view(signed).copy()).cuda()
    view = base[:, :half]
    assert not view.is_contiguous()
    torch.cuda.synchronize()
    async with loopback() as (server, client):
        fut = post(server, case, 9)
        await server.aflush()
        await client.asend(view, 9)
        assert tuple(await fut) == (9, case.nbytes)
        case.check_against(case.expected, "rows sender")
        assert np.array_equal(base.cpu().numpy(), host.view(signed)), \
            "source changed"


@modes
async def test_element_misaligned_source(dst, src, acc):
    """The message behind a uint8 view at byte offset 1."""
    case = GuardedCast(660, dst, src, 4097, accumulate=acc)
    raw = np.zeros(case.nbytes + 16, dtype=np.uint8)
    raw[1:1 + case.nbytes] = case.src_words.view(np.uint8)
    dev = torch.from_numpy(raw.copy()).cuda()
    view = dev[1:1 + case.nbytes]
    assert view.data_ptr() % itemsize(src) == 1
    torch.cuda.synchronize()
    async with loopback() as (server, client):
        fut = post(server, case, 10)
        await server.aflush()
        await client.asend(view, 10)
        assert tuple(await fut) == (10, case.nbytes)
        case.check_against(case.expected, "misaligned source")
        assert np.array_equal(dev.cpu().numpy(), raw), "source changed"


# -- prefix, zero length ----------------------------------------------------------


@modes
async def test_prefix_and_zero_length(dst, src, acc):
    n = (64 << 10) // itemsize(src) + 1
    case = GuardedCast(670, dst, src, n, accumulate=acc, dst_cap=2 * n)
    async with loopback() as (server, client):
        assert case.dst_view.numel() == 2 * n
        fut = post(server, case, 11)
        await server.aflush()
        await client.asend(case.src_view, 11)
        assert tuple(await fut) == (11, case.nbytes)
        case.check("prefix")  # the second half is unchanged
        fut = post(server, case, 12)
        await server.aflush()
        await client.asend(np.zeros(0, dtype=np.uint8), 12)
        assert tuple(await fut) == (12, 0)
        case.check("after a zero-length message")


# -- failures ---------------------------------------------------------------------


@pytest.mark.parametrize("dst,src", [NARROW, WIDEN],
                         ids=["f32-to-bf16", "bf16-to-f32"])
async def test_truncated_then_msg_dtype_in_that_order(dst, src):
    ms = itemsize(src)
    async with loopback() as (server, client):
        n = (128 << 10) // ms
        cap = n * ms  # the buffer's capacity in message bytes
        junk = torch.ones(cap + 3 * ms, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        # Rendezvous sizes: both sides fail. One element too many, first
        # whole, then with a ragged byte: too long comes first.
        for k, length in enumerate([cap + ms, cap + ms + 1]):
            case = GuardedCast(680 + k, dst, src, n, accumulate=bool(k))
            fut = post(server, case, 13)
            await server.aflush()
            send = client.asend(junk[:length], 13)
            with pytest.raises(Exception, match="truncated") as e:
                await fut
            assert str(length) in str(e.value) and str(cap) in str(e.value)
            with pytest.raises(Exception, match="truncated"):
                await send
            case.check_untouched(f"too long ({length} B)")
            await plain_message_still_delivered(server, client)
        # Not longer than the buffer, but not whole elements.
        for k, length in enumerate([cap - 1, cap + 1] if ms == 2
                                   else [cap - 1, cap + 3]):
            case = GuardedCast(684 + k, dst, src, n, accumulate=bool(k))
            fut = post(server, case, 14)
            await server.aflush()
            send = client.asend(junk[:length], 14)
            with pytest.raises(Exception, match="msg_dtype"):
                await fut
            with pytest.raises(Exception, match="msg_dtype"):
                await send
            case.check_untouched(f"ragged ({length} B)")
            await plain_message_still_delivered(server, client)
        # A host sender (eager): only the receiver fails.
        small = GuardedCast(688, dst, src, 64)
        for length, what in [(64 * ms + ms, "truncated"),
                             (64 * ms - 1, "msg_dtype")]:
            fut = post(server, small, 15)
            await server.aflush()
            await client.asend(np.ones(length, dtype=np.uint8), 15)
            with pytest.raises(Exception, match=what):
                await fut
            small.check_untouched(f"eager, {what}")
            await plain_message_still_delivered(server, client)
        assert stats(server)["cast_rx"] == 0


async def test_cancel_leaves_the_buffer_untouched():
    case = GuardedCast(690, "float32", "bfloat16", 2048, accumulate=True)
    server = sw.Server()
    client = sw.Client()
    await client.aconnect_address(server.listen_address())
    fut = post(server, case, 17)
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
            for dt in (torch.float64, torch.int32, torch.uint8):
                buf = torch.zeros(64, dtype=dt, device="cuda")
                with pytest.raises(ValueError, match="^msg_dtype limit:.*dtype"):
                    end.arecv(buf, 0, 0, msg_dtype="bfloat16")
            big = torch.zeros(16, 32, dtype=torch.float32, device="cuda")
            with pytest.raises(ValueError,
                               match="^msg_dtype limit:.*contiguous"):
                end.arecv(big[:, :8], 0, 0, msg_dtype="bfloat16")
            with pytest.raises(ValueError,
                               match="^msg_dtype limit:.*contiguous"):
                end.arecv(big.t(), 0, 0, msg_dtype="float16")
            with pytest.raises(ValueError, match="^msg_dtype limit:.*index"):
                end.arecv(big, 0, 0, msg_dtype="bfloat16", index=[0, 1])
            raw = torch.zeros(64, dtype=torch.uint8, device="cuda")
            native = end._server if end is server else end._client
            shim = sw._norm_buffer(raw[1:33])  # fp32 data at an odd address
            with pytest.raises(ValueError, match="^msg_dtype limit:.*aligned"):
                native.recv(shim, 0, 0, None, None, dtype="float32",
                            msg_dtype="bfloat16")
            with pytest.raises(ValueError, match="^msg_dtype limit:.*int32"):
                end.arecv(big, 0, 0, msg_dtype="int32")
        torch.cuda.synchronize()
        assert not big.any() and not raw.any()


async def test_equal_dtypes_are_the_ordinary_receive():
    """msg_dtype equal to the buffer's dtype: today's receive, plain or
    reducing, and no cast_rx."""
    from _guard_accum import GuardedAccum

    async with loopback() as (server, client):
        plain_src = torch.arange(1000, dtype=torch.float32, device="cuda")
        plain_dst = torch.zeros(1000, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        fut = server.arecv(plain_dst, 20, FULL, msg_dtype=torch.float32)
        await server.aflush()
        await client.asend(plain_src, 20)
        assert tuple(await fut) == (20, 4000)
        torch.cuda.synchronize()
        assert torch.equal(plain_src, plain_dst)
        case = GuardedAccum(700, "bfloat16", 4096)
        fut = server.arecv(case.dst_view, 21, FULL, reduce="sum",
                           msg_dtype="bfloat16")
        await server.aflush()
        await client.asend(case.src_view, 21)
        assert tuple(await fut) == (21, 4096)
        case.check("equal dtypes, reducing")
        s = stats(server)
        assert s["cast_rx"] == 0 and s["reduce_rx"] == 1


# -- cross-process over hipIpc ---------------------------------------------------------

IPC_ELEMS = (256 << 10) + 5


def _ipc_cases():
    return [GuardedCast(710, "float32", "bfloat16", IPC_ELEMS,
                        accumulate=True, src_off=16),
            GuardedCast(711, "bfloat16", "float32", IPC_ELEMS)]


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
        for k, case in enumerate(cases):
            await server.asend(ep, case.src_view, k)
        await server.aflush_ep(ep)
        ok = True
        for case in cases:
            try:
                case.check_source("child")
            except AssertionError:
                ok = False
        verdict.value = int(ok)
        await server.aclose()

    asyncio.run(inner())


async def test_cross_process_ipc(port):
    """The child (a fresh process) sends contiguous device messages; the
    convert kernel reads the hipIpc mapping in place."""
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
        futs = [post(client, case, k) for k, case in enumerate(cases)]
        for k, case in enumerate(cases):
            assert tuple(await futs[k]) == (k, case.nbytes)
        for case in cases:
            case.check_against(case.expected,
                               f"hipIpc {case.src_dtype}->{case.dst_dtype}")
        s = stats(client)
        assert s["cast_rx"] == 2 and s["reduce_rx"] == 1
        await client.aclose()
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            p.join()
        p.close()
    assert verdict.value == 1, "child: a source arena changed or child failed"
