"""Routes through the GPU layer's begin_pull / begin_h2d / begin_d2h that no
other module drives: the SDMA pull engine, a strided source on the
device-to-host staging download, two row-strided sides that disagree, and
the geometry refusals of a row-strided receive window.

Delivery is a byte-exact copy; the transfers run through tests/_guard_nd.py
(numpy reference, whole destination arena compared). STARWAY_PULL and
STARWAY_FORCE_XHOST are read once per process, so those cases get a fresh
child each.

Where the other routes are driven (destination x source):
  host x contiguous / rows / N-D    test_gpu.py::test_gpu_to_cpu_recv,
      ::test_strided_device_to_host_recv,
      test_gpu_nd.py::test_nd_device_source_to_host_receive
  dense device x contiguous / rows / N-D
      test_gpu.py::test_device_send_recv_same_process (batched when small:
      ::test_batched_small_pulls_exact),
      ::test_strided_send_to_contiguous_recv,
      test_gpu_nd.py::test_transposed_source_to_contiguous
  rows window x contiguous / rows / N-D
      test_gpu.py::test_contiguous_send_to_strided_recv_above_inbox_size,
      ::test_strided_to_strided_roundtrip,
      test_gpu_nd.py::test_nd_source_to_2d_row_strided_destination
  N-D window x contiguous / N-D
      test_gpu_nd.py::test_contiguous_to_permuted_3d_window,
      ::test_nd_to_nd_different_shapes
  reducing x contiguous / rows and N-D / element-misaligned
      test_gpu_reduce.py::test_rendezvous_preposted, ::test_strided_sources,
      ::test_element_misaligned_source
  begin_h2d into dense / rows / N-D / reducing
      test_gpu.py::test_cpu_to_gpu_recv,
      ::test_host_send_to_strided_device_recv,
      test_gpu_nd.py::test_host_send_to_nd_device_receive,
      test_gpu_reduce.py::test_host_sender
"""
import asyncio
import contextlib
import multiprocessing as mp
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")
import torch  # noqa: E402

import starway_amd as sw  # noqa: E402

from _guard_nd import GuardedNd, View  # noqa: E402

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


async def _deliver(server, client, case, tag, label):
    fut = server.arecv(case.dst_view, tag, FULL)
    await client.asend(case.src_view, tag)
    await client.aflush()
    got_tag, length = await fut
    assert (got_tag, length) == (tag, case.src.nbytes), label
    case.check(label)


def _child(body, env, q):
    import os

    os.environ.update(env)  # read at first use, after the imports above
    try:
        asyncio.run(asyncio.wait_for(body(), timeout=120))
        q.put("ok")
    except BaseException:  # noqa: BLE001 - the parent reports it
        q.put(traceback.format_exc())


def _run_in_child(body, env):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(body, env, q))
    p.start()
    try:
        assert q.get(timeout=180) == "ok"
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            p.join()
        p.close()


# 8205 B: off the inbox ring (4 KiB), odd length, destination 3 B off its
# 256 B allocation alignment.
FLAT = View.dense(0, (8205,), 1)
FLAT_OFF3 = View.dense(3, (8205,), 1)
# 12 rows of 96 B, 160 B apart.
ROWS = View(32, (12, 48), (160, 2), 2)
# A (40, 24) int16 matrix stored transposed, 4 spare elements per stored row.
TRANSPOSED = View(0, (40, 24), (2, 88), 2)


async def _sdma_body():
    async with loopback() as (server, client):
        rx0 = server._server.get_stats()["gpu_rx"]
        await _deliver(server, client, GuardedNd(31, FLAT, FLAT_OFF3), 71,
                       "sdma: contiguous -> contiguous")
        # The strided routes do not consult the knob.
        await _deliver(server, client,
                       GuardedNd(32, ROWS, View.dense(0, ROWS.shape, 2)), 72,
                       "sdma: rows -> contiguous")
        assert server._server.get_stats()["gpu_rx"] == rx0 + 2


def test_sdma_pull_engine():
    """STARWAY_PULL=sdma: a flat device-to-device pull goes through
    hipMemcpyAsync instead of the copy kernel."""
    _run_in_child(_sdma_body, {"STARWAY_PULL": "sdma"})


async def _xhost_body():
    async with loopback() as (server, client):
        await _deliver(server, client, GuardedNd(36, FLAT, FLAT_OFF3), 70,
                       "d2h: contiguous source -> device")
        await _deliver(server, client,
                       GuardedNd(33, ROWS, View.dense(0, ROWS.shape, 2)), 73,
                       "d2h: rows source -> device")
        await _deliver(server, client,
                       GuardedNd(34, TRANSPOSED,
                                 View.dense(0, TRANSPOSED.shape, 2),
                                 dst_on_host=True), 74,
                       "d2h: N-D source -> host")


def test_strided_sources_through_the_host_staging_download():
    """STARWAY_FORCE_XHOST=1: a device send is downloaded to host staging
    (begin_d2h) and shipped eager; a rows source takes the 2-D download, an
    N-D source packs through device staging first."""
    _run_in_child(_xhost_body, {"STARWAY_FORCE_XHOST": "1"})


async def test_rows_sides_of_equal_size_but_different_geometry_are_refused():
    """8 rows of 64 B into 16 rows of 32 B: same 512 B, refused by the pull
    with its own text, on both sides; nothing is written."""
    async with loopback() as (server, client):
        a = torch.randint(1, 256, (8, 256), dtype=torch.uint8, device="cuda")
        b = torch.zeros(16, 256, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fut = server.arecv(b[:, :32], 0, 0)
        sfut = client.asend(a[:, :64], 76)
        with pytest.raises(Exception, match="row geometry mismatch"):
            await fut
        with pytest.raises(Exception, match="row geometry mismatch"):
            await sfut
        torch.cuda.synchronize()
        assert b.eq(0).all()


async def test_rendezvous_shorter_than_a_rows_window_gets_the_geometry_text():
    """8 KiB (off the inbox ring) into a 128 x 128 B window: the pull
    refuses it with the geometry text, not the truncation text."""
    async with loopback() as (server, client):
        src = torch.ones(8192, dtype=torch.uint8, device="cuda")
        frame = torch.zeros(128, 256, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fut = server.arecv(frame[:, :128], 0, 0)
        sfut = client.asend(src, 77)
        with pytest.raises(Exception, match="geometry mismatch"):
            await fut
        with pytest.raises(Exception, match="geometry mismatch"):
            await sfut
        torch.cuda.synchronize()
        assert frame.eq(0).all()


async def test_short_unexpected_host_message_into_a_rows_window_fails():
    """128 host bytes arrive before the receive into frame[:, :32] of an
    (8, 256) frame (256 B) is posted: refused like on every other plane,
    and nothing is written."""
    async with loopback() as (server, client):
        frame = torch.zeros(8, 256, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sentinel = np.zeros(1, dtype=np.uint8)
        sent = server.arecv(sentinel, 99, FULL)
        await server.aflush()
        await client.asend(np.full(128, 7, dtype=np.uint8), 78)
        await client.asend(np.ones(1, dtype=np.uint8), 99)
        await sent  # the message ahead of it is parsed and staged
        with pytest.raises(Exception, match="geometry|truncated"):
            await server.arecv(frame[:, :32], 78, FULL)
        torch.cuda.synchronize()
        assert frame.eq(0).all()
