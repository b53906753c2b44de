#!/usr/bin/env python3
"""Driver-contract benchmark for starway_amd.

Headline metric (BASELINE.json): aggregate GB/s of tagged all-pairs
send/recv of HIP device tensors over xGMI, at N MI355X endpoints
(one process per GPU), plus 64 B pingpong half-RTT latency.

One "step" = every rank tag-sends a fixed per-rank byte volume
(``--msg-bytes``, default 256 MiB), split evenly across all peers, and
receives the matching inbound messages (weak scaling: per-GPU work is fixed
as N grows). N=1 runs a same-process loopback pair on cuda:0 (HBM-bound);
N>=2 is xGMI-bound. With no CUDA device the bench falls back to CPU numpy
buffers over localhost TCP (small default size) so it stays runnable
anywhere.

Launch (driver): N=1 plain; N>1 via
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
torch.distributed (gloo) is used ONLY for rank rendezvous (worker-address
exchange + barriers); the data plane is starway_amd itself.

Rank 0 prints ONE JSON line with the aggregate result.

A plain run only sets up, warms up, times ``--steps`` steps and prints the
result line. ``--full`` adds the 64 B pingpong latency probes (asyncio and
raw-callback API) after the timed region and reports them in ``config``.
``--dump-outputs DIR`` writes what the last timed step delivered (each
rank's receive buffers, or a fixed seeded sample of them) to
``DIR/<name>.npy`` as float32; send payloads are seeded, so two builds run
with the same arguments can be compared output for output.
"""
from __future__ import annotations

import os

# ROCm multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues
# (default 4); oversubscription time-slices co-mapped streams at ~ms
# granularity. Must be set before the FIRST HIP init in the process
# (torch's or ours) — see ROUND2_NOTES.md "hardware-queue starvation".
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import argparse
import asyncio
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

import numpy as np  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser(description="starway_amd driver benchmark")
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--msg-bytes", type=int, default=256 * 1024 * 1024,
                   help="per-rank outbound bytes per step (split across peers)")
    p.add_argument("--chunks", type=int, default=None,
                   help="tagged messages per peer per step (default: 1 on "
                        "GPU — chunking adds per-message future overhead "
                        "that the serialized same-pair kernels cannot hide "
                        "(measured); 4 on CPU where CMA/ring streaming "
                        "pipelines across chunks, +50%%)")
    p.add_argument("--inflight", type=int, default=2,
                   help="outstanding steps in the timed region (pipelined "
                        "tagged rounds; 1 = strictly sequential). All K "
                        "steps complete inside the timed window (drained "
                        "before the closing sync/barrier).")
    p.add_argument("--lat-iters", type=int, default=200,
                   help="64B pingpong iterations for the latency probe "
                        "(runs only with --full)")
    p.add_argument("--full", action="store_true",
                   help="also run the 64B pingpong latency probes after the "
                        "timed steps (off by default: a plain run measures "
                        "only the headline bandwidth)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write the buffers the last "
                        "step delivered to DIR/<name>.npy (float32; a fixed "
                        "seeded sample when they exceed the size budget)")
    p.add_argument("--device", default=None,
                   help="force 'cpu' or 'cuda' (default: auto)")
    p.add_argument("--transport", choices=("p2p", "rccl"), default="p2p",
                   help="p2p: starway tagged engine (hipIpc pulls); "
                        "rccl: ncclSend/ncclRecv all-to-all groups")
    p.add_argument("--json-out", default=None)
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")
    if args.warmup < 0:
        p.error("--warmup must be >= 0")
    return args


def make_tag(src_rank: int, step: int, chunk: int = 0) -> int:
    return (1 << 60) | (src_rank << 40) | ((chunk & 0xFF) << 32) | (
        step & 0xFFFFFFFF)


LAT_TAG_BASE = 1 << 59

PAYLOAD_SEED = 0x5EED
DUMP_SEED = 0xD0C5
# --dump-outputs budget for the whole job, in float32 elements: 32 MiB of
# .npy payload, split evenly over ranks and then over each rank's buffers.
DUMP_MAX_ELEMS = 8 << 20


def make_payload(n: int, src_rank: int, dst_rank: int, device: str):
    """Seeded uint8 send payload for the (src, dst) pair: identical from run
    to run for the same arguments, different for every pair and position so
    a misrouted or shifted delivery shows up in the dumped outputs."""
    seed = PAYLOAD_SEED + src_rank * 4099 + dst_rank
    if device == "cpu":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda",
                         generator=g)


def sample_indices(n: int, k: int):
    """Sorted positions of the fixed seeded sample of an n-element buffer
    that --dump-outputs keeps, or None when the whole buffer fits in k."""
    if n <= k:
        return None
    return np.sort(np.random.default_rng(DUMP_SEED).integers(
        0, n, k, dtype=np.int64))


def dump_outputs(out_dir: str, named: dict, device: str, max_elems: int):
    """Write each named 1-D uint8 buffer (or its seeded sample) as
    out_dir/<name>.npy in float32."""
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    per_buf = max(1, max_elems // max(1, len(named)))
    for name, buf in named.items():
        idx = sample_indices(int(buf.shape[0]), per_buf)
        if device == "cpu":
            a = buf if idx is None else buf[idx]
        else:
            import torch

            t = buf if idx is None else buf[torch.from_numpy(idx).cuda()]
            a = t.cpu().numpy()
        np.save(out / f"{name}.npy", a.astype(np.float32))


async def run_rank(args, rank: int, world: int, device: str, dist):
    import starway_amd as sw

    full_mask = (1 << 64) - 1
    n_peers = max(1, world - 1)
    per_peer = args.msg_bytes // n_peers if world > 1 else args.msg_bytes

    def alloc(n, fill=None):
        if device == "cpu":
            a = np.empty(n, dtype=np.uint8)
            if fill is not None:
                a.fill(fill)
            return a
        import torch

        t = torch.empty(n, dtype=torch.uint8, device="cuda")
        if fill is not None:
            t.fill_(fill)
        return t

    def sync_device():
        if device != "cpu":
            import torch

            torch.cuda.synchronize()

    server = sw.Server()
    blob = server.listen_address()

    if world > 1:
        blobs = [None] * world
        dist.all_gather_object(blobs, blob)
        # rank i's client[j] connects to rank j's server (full mesh).
        clients = {}
        for j in range(world):
            if j == rank:
                continue
            c = sw.Client()
            await c.aconnect_address(blobs[j])
            clients[j] = c
        dist.barrier()
        peers = sorted(clients.keys())
    else:
        c = sw.Client()
        await c.aconnect_address(blob)
        clients = {0: c}
        peers = [0]

    chunks = max(1, min(args.chunks, per_peer))
    bounds = [per_peer * k // chunks for k in range(chunks + 1)]
    send_bufs = {j: make_payload(per_peer, rank, j, device) for j in peers}
    send_views = {j: [send_bufs[j][bounds[k]:bounds[k + 1]]
                      for k in range(chunks)] for j in peers}
    # Recv buffers are double-buffered by step parity so pipelined steps
    # (inflight > 1) never write the same destination concurrently; send
    # buffers are immutable after the fill, so one copy suffices.
    recv_bufs = [{j: alloc(per_peer) for j in peers} for _ in range(2)]
    recv_views = [
        {j: [recv_bufs[par][j][bounds[k]:bounds[k + 1]]
             for k in range(chunks)] for j in peers}
        for par in range(2)
    ]
    sync_device()

    mesh = None
    if args.transport == "rccl":
        if device == "cpu":
            raise SystemExit("--transport rccl needs GPUs")
        import torch

        from starway_amd import rccl as swr

        if world > 1:
            uid = [swr.unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)
            uid = uid[0]
        else:
            uid = swr.unique_id()
        mesh = swr.RcclMesh(uid, rank=rank, world=world,
                            device=torch.cuda.current_device())
        # all-to-all layout: peer-major chunks, msg_bytes per rank total.
        chunk = args.msg_bytes // world
        rccl_send = make_payload(chunk * world, rank, world, device)
        rccl_recv = alloc(chunk * world)
        sync_device()

    def begin_step(step_idx: int):
        if mesh is not None:
            mesh.all_to_all(rccl_send, rccl_recv)
            return None
        rv = recv_views[step_idx & 1]
        recvs = [
            server.arecv(rv[j][k], make_tag(j, step_idx, k), full_mask)
            for j in peers for k in range(chunks)
        ]
        sends = [
            clients[j].asend(send_views[j][k], make_tag(rank, step_idx, k))
            for j in peers for k in range(chunks)
        ]
        return asyncio.gather(*sends, *recvs)

    async def run_steps(first: int, count: int, inflight: int):
        if mesh is not None:
            for i in range(count):
                begin_step(first + i)
                mesh.synchronize()
            return
        pending: list = []
        for i in range(count):
            pending.append(begin_step(first + i))
            if len(pending) >= inflight:
                await pending.pop(0)
        for fut in pending:
            await fut

    inflight = max(1, args.inflight)

    # ---- warmup ----
    await run_steps(0, args.warmup, inflight)
    sync_device()
    if world > 1:
        dist.barrier()

    # ---- timed region: K pipelined steps, fully drained before the
    # closing sync (every byte of all K steps moves inside the window) ----
    t0 = time.perf_counter()
    await run_steps(args.warmup, args.steps, inflight)
    sync_device()
    elapsed = time.perf_counter() - t0
    if world > 1:
        import torch

        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        dist.barrier()

    # ---- outputs of the last timed step (what a caller received) ----
    if args.dump_outputs:
        if mesh is not None:
            named = {f"rank{rank}_alltoall_recv": rccl_recv}
        else:
            last = recv_bufs[(args.warmup + args.steps - 1) & 1]
            named = {f"rank{rank}_recv_from{j}": last[j] for j in peers}
        dump_outputs(args.dump_outputs, named, device,
                     DUMP_MAX_ELEMS // world)
        if world > 1:
            dist.barrier()

    # ---- 64 B pingpong latency probe (rank0 <-> rank1, or loopback);
    # --full only ----
    half_rtt_us = None
    lat_samples = []
    ping = alloc(64, fill=1) if args.full else None
    pong = alloc(64) if args.full else None
    if not args.full:
        pass  # plain run: headline bandwidth only
    elif world == 1:
        for i in range(args.lat_iters):
            t1 = time.perf_counter()
            fut = server.arecv(pong, LAT_TAG_BASE + i, full_mask)
            await clients[0].asend(ping, LAT_TAG_BASE + i)
            await fut
            lat_samples.append(time.perf_counter() - t1)
    elif rank in (0, 1):
        other = 1 - rank
        for i in range(args.lat_iters):
            if rank == 0:
                t1 = time.perf_counter()
                fut = server.arecv(pong, make_tag(other, 1 << 30 | i), full_mask)
                await clients[other].asend(ping, make_tag(rank, 1 << 30 | i))
                await fut
                lat_samples.append(time.perf_counter() - t1)
            else:
                await server.arecv(pong, make_tag(other, 1 << 30 | i), full_mask)
                await clients[other].asend(ping, make_tag(rank, 1 << 30 | i))
    if lat_samples:
        half_rtt_us = float(np.percentile(np.array(lat_samples) * 1e6, 50)) / 2.0

    # Raw-callback latency variant (N=1 only): the same 64 B tagged
    # delivery through the public callback API (reference surface too),
    # with a GIL-yielding wait instead of an asyncio future — isolates the
    # event-loop wakeup cost from the transport cost.
    half_rtt_raw_us = None
    if args.full and world == 1:
        raw_samples = []
        for i in range(args.lat_iters):
            done: list = []
            t1 = time.perf_counter()
            server.recv(pong, LAT_TAG_BASE + (1 << 28) + i, full_mask,
                        lambda tag, ln: done.append(1),
                        lambda err: done.append(err))
            sent: list = []
            clients[0].send(ping, LAT_TAG_BASE + (1 << 28) + i,
                            lambda: sent.append(1),
                            lambda err: sent.append(err))
            while not done:
                time.sleep(0)
            raw_samples.append(time.perf_counter() - t1)
            while not sent:
                time.sleep(0)
        half_rtt_raw_us = float(
            np.percentile(np.array(raw_samples) * 1e6, 50)) / 2.0

    if world > 1:
        dist.barrier()

    # ---- teardown ----
    for c in clients.values():
        await c.aclose()
    await server.aclose()

    return elapsed, half_rtt_us, half_rtt_raw_us


def main() -> int:
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    device = args.device
    if device is None:
        try:
            import torch

            device = "cuda" if torch.cuda.is_available() else "cpu"
        except ImportError:
            device = "cpu"
    if device == "cpu" and args.msg_bytes > 64 * 1024 * 1024:
        # CPU/TCP fallback: keep the default run snappy.
        args.msg_bytes = 16 * 1024 * 1024
    if args.chunks is None:
        args.chunks = 1 if device == "cuda" else 4
    if device == "cuda":
        import torch

        if world > torch.cuda.device_count():
            # Multiple ranks share a GPU (emulation): cap pull streams so
            # the per-device HSA queue count stays under the hardware
            # budget — oversubscribed queues are time-sliced at ~ms
            # granularity (measured: 8 ranks x 8 lanes on one GPU ran 38x
            # slower than lanes=1). The real 1-process-per-GPU topology
            # keeps the default 8 lanes.
            os.environ.setdefault("STARWAY_LANES", "1")
            os.environ.setdefault("STARWAY_SM_LANES", "1")

    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist_mod

        dist = dist_mod
        if device == "cuda":
            # modulo so a 2-rank run on a 1-GPU box exercises the full
            # cross-process hipIpc path (the driver's 8-GPU run has 1:1).
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
        dist.init_process_group("gloo")

    elapsed, half_rtt_us, half_rtt_raw_us = asyncio.run(
        run_rank(args, rank, world, device, dist))

    if rank == 0:
        n_peers = max(1, world - 1)
        per_peer = args.msg_bytes // n_peers if world > 1 else args.msg_bytes
        moved_per_rank = per_peer * (n_peers if world > 1 else 1)
        total_bytes = world * moved_per_rank * args.steps
        gbps = total_bytes / elapsed / 1e9
        result = {
            "metric": "tagged_allpairs_bandwidth",
            "value": round(gbps, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 6),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "uint8",
            "data": "synthetic",
            "config": {
                "model": "tagged-pingpong-allpairs",
                "message_bytes_per_rank": args.msg_bytes,
                "message_bytes_per_peer": args.msg_bytes // max(1, world - 1),
                "chunks_per_peer": args.chunks,
                "inflight_steps": args.inflight,
                "endpoints": world,
                "device": device,
                "transport": args.transport,
                "parallelism": f"p2p-mesh{world}",
                "full": args.full,
                "pingpong_64B_half_rtt_us":
                    round(half_rtt_us, 2) if half_rtt_us else None,
                "pingpong_64B_half_rtt_us_raw_api":
                    round(half_rtt_raw_us, 2) if half_rtt_raw_us else None,
                "note": "N=1 is same-GPU loopback (HBM-bound); N>=2 is "
                        "xGMI-bound; value counts each sent byte once",
            },
        }
        line = json.dumps(result)
        print(line, flush=True)
        if args.json_out:
            Path(args.json_out).write_text(line + "\n")

    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
