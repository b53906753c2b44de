"""Engine-level doorbell scenarios over loopback, guard-banded and exact.

STARWAY_DOORBELL=1 is read once per process, so the scenarios run in
spawned children (three in this file); each child returns one verdict per
scenario through a queue, and the parent kills a child that overruns.

Doorbell delivery is opportunistic -- whether the pre-armed kernel or the
batched unpack path delivers a message depends on timing -- so bytes,
lengths, tags and counters are asserted always, and doorbell participation
only as `doorbell_rx > 0` over a whole pre-posted run. The scenarios aim
the engine's conflict paths (steal_armed, armed_done_, the nomatch
fallthrough in handle_smsg, the expiry streak and back-off in
progress_armed); whichever path a run takes, the outcome must be the same.
(The wait kernel's own status words: tests/test_inbox_kernels.py.)
"""
import asyncio
import contextlib
import multiprocessing as mp
import traceback

import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

ALL = (1 << 64) - 1


@contextlib.asynccontextmanager
async def _loopback():
    import starway_amd as sw

    server = sw.Server()
    client = sw.Client()
    await client.aconnect_address(server.listen_address())
    try:
        await asyncio.sleep(0.3)  # cold-start probe settle (stats asserts)
        yield server, client, next(iter(server.list_clients()))
    finally:
        await client.aclose()
        await server.aclose()


def _case(seed, nbytes, src_off=0, dst_off=0, **kw):
    from _guard import GuardedCopy, Region

    return GuardedCopy(seed, Region.flat(src_off, nbytes),
                       Region.flat(dst_off, nbytes), **kw)


def _untouched(case, label):
    import numpy as np

    got = case._fetch(case.dst_buf)
    assert np.array_equal(got, case.dst_host), f"{label}: arena written"


def _stats(server, client):
    return server._server.get_stats(), client._client.get_stats()


# -- scenarios ----------------------------------------------------------------


async def _preposted_pingpong():
    """Sizes around the 16 B path's edges and the slot's end, destination
    offsets 0 and 3; every iteration on fresh arenas."""
    async with _loopback() as (server, client, ep):
        msgs = 0
        for size in [1, 15, 16, 17, 4095, 4096]:
            for off in [0, 3]:
                for it in range(4):
                    seed = 70_000 + size * 64 + off * 8 + it
                    ping = _case(seed, size, src_off=it % 2, dst_off=off)
                    pong = _case(seed + 4, size, src_off=off, dst_off=off)
                    sfut = server.arecv(ping.dst_view, 1, ALL)
                    await asyncio.sleep(0)
                    await client.asend(ping.src_view, 1)
                    assert tuple(await sfut) == (1, size)
                    cfut = client.arecv(pong.dst_view, 2, ALL)
                    await asyncio.sleep(0)
                    await server.asend(ep, pong.src_view, 2)
                    assert tuple(await cfut) == (2, size)
                    ping.check(f"ping {size} B dst+{off} iter {it}")
                    pong.check(f"pong {size} B dst+{off} iter {it}")
                    msgs += 1
        ss, cs = _stats(server, client)
        assert ss["inbox_rx"] == msgs and cs["inbox_rx"] == msgs, (ss, cs)
        assert ss["doorbell_rx"] <= ss["inbox_rx"]
        assert cs["doorbell_rx"] <= cs["inbox_rx"]
        rang = ss["doorbell_rx"] + cs["doorbell_rx"]
        assert rang > 0, "no pre-posted message was delivered by a doorbell"
        return {"messages_per_side": msgs, "doorbell_rx": rang}


async def _nomatch_fallthrough():
    """An exact-tag recv is armed; the next message carries another tag.
    The doorbell must leave it in its slot (parked as unexpected), the
    armed recv must still get its own message, and a later recv must get
    the parked one. Three arming delays: the doorbell is queued, resident,
    or past its expiry streak when the foreign tag lands."""
    async with _loopback() as (server, client, ep):
        for k, delay in enumerate([0, 0.001, 0.010]):
            one = _case(71_000 + k, 300 + k, dst_off=3)
            two = _case(71_010 + k, 200 + k, src_off=1)
            fut1 = server.arecv(one.dst_view, 1, ALL)
            await asyncio.sleep(delay)
            await client.asend(two.src_view, 2)
            await client.asend(one.src_view, 1)
            assert tuple(await fut1) == (1, 300 + k)
            one.check(f"armed tag-1 recv, delay {delay}")
            _untouched(two, "tag-2 arena before its recv")
            assert tuple(await server.arecv(two.dst_view, 2, ALL)) == (
                2, 200 + k)
            two.check(f"parked tag-2 message, delay {delay}")
        ss, _ = _stats(server, client)
        assert ss["inbox_rx"] == 6, ss
        return {"doorbell_rx": ss["doorbell_rx"]}


async def _oversize_into_armed_recv():
    async with _loopback() as (server, client, ep):
        for k, delay in enumerate([0, 0.001]):
            big = _case(72_000 + k, 128)
            small = _case(72_010 + k, 64, dst_off=3 * k)
            fut = server.arecv(small.dst_view, 0, 0)
            await asyncio.sleep(delay)
            send = client.asend(big.src_view, 5)
            with pytest.raises(Exception, match="message truncated"):
                await fut
            await send  # eager semantics: the push itself completes
            _untouched(small, f"oversize into armed recv, delay {delay}")
        return {}


async def _short_message():
    """100 B into a 256 B buffer: length 100, and only 100 bytes change."""
    async with _loopback() as (server, client, ep):
        for k, (off, delay) in enumerate([(0, 0), (3, 0), (0, 0.001)]):
            case = _case(73_000 + k, 100, src_off=k, dst_off=off)
            start = case.dst.start
            buf = case.dst_buf[start:start + 256]  # ends inside the guard
            assert buf.numel() == 256
            fut = server.arecv(buf, 9, ALL)
            await asyncio.sleep(delay)
            await client.asend(case.src_view, 9)
            assert tuple(await fut) == (9, 100)
            case.check(f"short message dst+{off} delay {delay}")
        ss, _ = _stats(server, client)
        assert ss["inbox_rx"] == 3, ss
        return {"doorbell_rx": ss["doorbell_rx"]}


async def _expiry_and_backoff():
    """Idle for 50 ms with a recv posted: the doorbell expires three times
    and stands down. The message must still arrive exactly, and the
    doorbell path must keep working for ten pre-posted iterations."""
    async with _loopback() as (server, client, ep):
        first = _case(74_000, 512, dst_off=1)
        fut = server.arecv(first.dst_view, 3, ALL)
        await asyncio.sleep(0.05)
        await client.asend(first.src_view, 3)
        assert tuple(await fut) == (3, 512)
        first.check("after the expiry streak")
        for it in range(10):
            case = _case(74_001 + it, 64 + it, dst_off=it % 4)
            fut = server.arecv(case.dst_view, 3, ALL)
            await asyncio.sleep(0)
            await client.asend(case.src_view, 3)
            assert tuple(await fut) == (3, 64 + it)
            case.check(f"pre-posted iteration {it} after back-off")
        ss, _ = _stats(server, client)
        assert ss["inbox_rx"] == 11 and ss["doorbell_rx"] <= 11, ss
        return {"doorbell_rx": ss["doorbell_rx"]}


async def _steal_by_another_plane():
    """A wildcard device recv is armed; a host (numpy) eager send matches
    it first, so the engine must take the recv back from the doorbell.
    The device small send that follows goes to a new recv. One inbox
    delivery per pair, each payload exactly once."""
    async with _loopback() as (server, client, ep):
        for k, delay in enumerate([0, 0.001, 0.010]):
            host = _case(75_000 + k, 96, dst_off=3, src_on_host=True)
            dev = _case(75_010 + k, 96, src_off=1)
            rx0 = server._server.get_stats()["inbox_rx"]
            fut = server.arecv(host.dst_view, 0, 0)
            await asyncio.sleep(delay)
            await client.asend(host.src_view, 21)
            assert tuple(await fut) == (21, 96)
            host.check(f"host eager send into the armed recv, delay {delay}")
            _untouched(dev, "device arena before its recv")
            fut = server.arecv(dev.dst_view, 0, 0)
            await asyncio.sleep(delay)
            await client.asend(dev.src_view, 22)
            assert tuple(await fut) == (22, 96)
            dev.check(f"device send after the steal, delay {delay}")
            host.check("first recv's arena after the second delivery")
            assert server._server.get_stats()["inbox_rx"] == rx0 + 1
        return {"doorbell_rx": server._server.get_stats()["doorbell_rx"]}


async def _second_recv_while_armed():
    """Two recvs posted, the first armed; two device sends in order must
    land in posting order."""
    async with _loopback() as (server, client, ep):
        for k, delay in enumerate([0, 0.001]):
            a = _case(76_000 + k, 128, dst_off=k)
            b = _case(76_010 + k, 77, src_off=1, dst_off=3)
            fa = server.arecv(a.dst_view, 0, 0)
            await asyncio.sleep(delay)
            fb = server.arecv(b.dst_view, 0, 0)
            await asyncio.sleep(delay)
            await client.asend(a.src_view, 31)
            await client.asend(b.src_view, 32)
            assert tuple(await fa) == (31, 128)
            assert tuple(await fb) == (32, 77)
            a.check(f"first posted recv, delay {delay}")
            b.check(f"second posted recv, delay {delay}")
        ss, _ = _stats(server, client)
        assert ss["inbox_rx"] == 4 and ss["doorbell_rx"] <= 4, ss
        return {"doorbell_rx": ss["doorbell_rx"]}


GROUPS = {
    "pingpong": [_preposted_pingpong],
    "mismatch": [_nomatch_fallthrough, _oversize_into_armed_recv,
                 _short_message],
    "conflict": [_expiry_and_backoff, _steal_by_another_plane,
                 _second_recv_while_armed],
}


# -- child / parent -----------------------------------------------------------


def _child(group, q):
    import os

    os.environ["STARWAY_DOORBELL"] = "1"  # opt-in; read at first use
    verdicts = {}
    for scenario in GROUPS[group]:
        try:
            info = asyncio.run(asyncio.wait_for(scenario(), timeout=60))
            verdicts[scenario.__name__] = ("ok", info)
        except BaseException:
            verdicts[scenario.__name__] = ("failed", traceback.format_exc())
    q.put(verdicts)


@pytest.mark.parametrize("group", list(GROUPS))
def test_doorbell_scenarios(group):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(group, q))
    p.start()
    try:
        verdicts = q.get(timeout=180)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            p.join()
        p.close()
    assert set(verdicts) == {s.__name__ for s in GROUPS[group]}
    for name, (state, info) in verdicts.items():
        print(f"{name}: {state} {info if state == 'ok' else ''}")
    failed = {n: i for n, (s, i) in verdicts.items() if s != "ok"}
    assert not failed, "\n".join(f"--- {n}\n{i}" for n, i in failed.items())
