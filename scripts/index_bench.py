#!/usr/bin/env python
"""Indexed send/recv: pool[idx] moved by the indexed kernel against the
gather-copy route a user writes without it.

In-process loopback (client -> server), per message size and page size, a
seeded random permutation of all pages as both index lists, the variants
alternated round by round in one process:

* ``indexed``     ``asend(pool, index=idx)`` into ``arecv(pool, index=idx)``:
                  one launch of k_copy_indexed, no temporary
* ``gather_copy`` ``tmp = pool.index_select(0, idx)``, send, receive into a
                  second temporary, ``pool.index_copy_(0, idx, tmp2)``: the
                  route without ``index=`` (the index tensors are already
                  on the device; the synchronise between index_select and
                  the send is needed, the engine pulls on its own stream)
* ``contiguous``  a contiguous send of the same bytes: the ceiling

Every call is timed to delivery on the host clock: from before the receive
is posted until both futures have resolved and the devices are
synchronised. Per variant: median over rounds of the mean time of
``--calls`` calls, and the spread (max - min over rounds, relative to the
median) inside this process; the run-to-run spread comes from repeating the
command. ``post_us`` is the part of an ``indexed`` call spent inside the two
posting calls (index validation and copy, on the caller's thread), median
over all timed calls. One JSON line per (pair, message, page).

``--kernel-only`` instead launches the indexed kernel (both sides indexed)
and the flat copy kernel ``--calls`` times each per point through the test
hooks, for a rocprofv3 --kernel-trace --stats run of its own; the bytes
each launch moves are printed so kernel time turns into bytes/s.

Needs a GPU; there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import asyncio
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FULL = (1 << 64) - 1
VARIANTS = ["indexed", "gather_copy", "contiguous"]


def make_point(torch, np, msg_bytes, page_bytes, src_dev, dst_dev, seed):
    count = msg_bytes // page_bytes
    rng = np.random.default_rng(seed)
    idx_s = rng.permutation(count).astype(np.int64)
    idx_d = rng.permutation(count).astype(np.int64)
    elems = page_bytes // 2
    p = {"count": count, "idx_s": idx_s, "idx_d": idx_d}
    with torch.cuda.device(src_dev):
        p["src_pool"] = torch.randn(count, elems, device="cuda",
                                    dtype=torch.float16)
        p["src_flat"] = torch.randn(count * elems, device="cuda",
                                    dtype=torch.float16)
        p["idx_s_dev"] = torch.from_numpy(idx_s).cuda()
    with torch.cuda.device(dst_dev):
        p["dst_pool"] = torch.zeros(count, elems, device="cuda",
                                    dtype=torch.float16)
        p["dst_flat"] = torch.zeros(count * elems, device="cuda",
                                    dtype=torch.float16)
        p["tmp2"] = torch.zeros(count, elems, device="cuda",
                                dtype=torch.float16)
        p["idx_d_dev"] = torch.from_numpy(idx_d).cuda()
    return p


async def bench_pair(args, torch, np, sw, src_dev, dst_dev, lines):
    def sync():
        torch.cuda.synchronize(src_dev)
        if dst_dev != src_dev:
            torch.cuda.synchronize(dst_dev)

    with torch.cuda.device(dst_dev):
        server = sw.Server()
    with torch.cuda.device(src_dev):
        client = sw.Client()
    await client.aconnect_address(server.listen_address())
    tag = 0
    try:
        for msg_mib in args.messages_mib:
            for page_kib in args.pages_kib:
                msg, page = msg_mib << 20, page_kib << 10
                if msg // page > 65536 or msg % page:
                    continue
                p = make_point(torch, np, msg, page, src_dev, dst_dev,
                               args.seed)
                sync()

                post_times = []

                async def indexed():
                    t0 = time.perf_counter()
                    fut = server.arecv(p["dst_pool"], tag, FULL,
                                       index=p["idx_d"])
                    sfut = client.asend(p["src_pool"], tag, index=p["idx_s"])
                    post_times.append(time.perf_counter() - t0)
                    await sfut
                    await fut
                    sync()

                async def gather_copy():
                    fut = server.arecv(p["tmp2"], tag, FULL)
                    tmp = p["src_pool"].index_select(0, p["idx_s_dev"])
                    torch.cuda.synchronize(src_dev)
                    await client.asend(tmp, tag)
                    await fut
                    p["dst_pool"].index_copy_(0, p["idx_d_dev"], p["tmp2"])
                    sync()

                async def contiguous():
                    fut = server.arecv(p["dst_flat"], tag, FULL)
                    await client.asend(p["src_flat"], tag)
                    await fut
                    sync()

                fns = {"indexed": indexed, "gather_copy": gather_copy,
                       "contiguous": contiguous}
                # Same result from both routes, at the size that is timed.
                await indexed()
                want = torch.empty_like(p["dst_pool"])
                want[p["idx_d_dev"]] = p["src_pool"][p["idx_s_dev"]].to(
                    want.device)
                same = bool(torch.equal(p["dst_pool"], want))
                p["dst_pool"].zero_()
                await gather_copy()
                same = same and bool(torch.equal(p["dst_pool"], want))
                del want
                for v in VARIANTS:
                    for _ in range(args.warmup):
                        await fns[v]()
                per_round = {v: [] for v in VARIANTS}
                post_times.clear()
                for r in range(args.rounds):
                    order = VARIANTS[r % 3:] + VARIANTS[:r % 3]
                    for v in order:
                        t0 = time.perf_counter()
                        for _ in range(args.calls):
                            await fns[v]()
                        per_round[v].append(
                            (time.perf_counter() - t0) / args.calls)
                rec = {"pair": [src_dev, dst_dev], "msg_mib": msg_mib,
                       "page_kib": page_kib, "pages": p["count"],
                       "rounds": args.rounds, "calls": args.calls,
                       "results_equal": same}
                for v in VARIANTS:
                    med = statistics.median(per_round[v])
                    rec[v] = {
                        "median_us": round(med * 1e6, 1),
                        "min_us": round(min(per_round[v]) * 1e6, 1),
                        "max_us": round(max(per_round[v]) * 1e6, 1),
                        "spread": round(
                            (max(per_round[v]) - min(per_round[v])) / med, 4),
                        "payload_gbps": round(msg / med / 1e9, 1),
                    }
                rec["indexed"]["post_us"] = round(
                    statistics.median(post_times) * 1e6, 1)
                rec["indexed_over_gather_copy"] = round(
                    rec["indexed"]["median_us"]
                    / rec["gather_copy"]["median_us"], 4)
                rec["indexed_over_contiguous"] = round(
                    rec["indexed"]["median_us"]
                    / rec["contiguous"]["median_us"], 4)
                # Faster by more than both spreads: even the slowest
                # indexed round beats the fastest gather-copy round.
                rec["indexed_wins_beyond_spread"] = (
                    rec["indexed"]["max_us"] < rec["gather_copy"]["min_us"])
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
                del p
    finally:
        await client.aclose()
        await server.aclose()


def kernel_only(args, torch, np, _core) -> None:
    for msg_mib in args.messages_mib:
        for page_kib in args.pages_kib:
            msg, page = msg_mib << 20, page_kib << 10
            if msg // page > 65536 or msg % page:
                continue
            p = make_point(torch, np, msg, page, 0, 0, args.seed)
            torch.cuda.synchronize()
            s, d = p["src_pool"].data_ptr(), p["dst_pool"].data_ptr()
            idx_s, idx_d = p["idx_s"].tolist(), p["idx_d"].tolist()
            for _ in range(args.calls):
                _core._copy_index_sync(d, idx_d, page, page, s, idx_s, page,
                                       page, msg, 0)
                _core._copy_device_sync(p["dst_flat"].data_ptr(),
                                        p["src_flat"].data_ptr(), msg, 0)
            print(json.dumps({"kernel_only": True, "msg_mib": msg_mib,
                              "page_kib": page_kib, "calls": args.calls,
                              "payload_bytes_per_launch": msg}), flush=True)
            del p


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--messages-mib", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--pages-kib", type=int, nargs="+",
                    default=[16, 64, 256, 2048])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import starway_amd as sw
    from starway_amd import _core

    if not sw.gpu_available():
        print("index_bench: no HIP device", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    if args.kernel_only:
        kernel_only(args, torch, np, _core)
        return 0
    if args.rounds < 5 or args.calls < 5:
        ap.error("at least 5 rounds of 5 calls")
    lines: list[str] = []
    pairs = [(0, 0)]
    if sw.gpu_device_count() >= 2:
        pairs.append((0, 1))
    for src_dev, dst_dev in pairs:
        asyncio.run(bench_pair(args, torch, np, sw, src_dev, dst_dev, lines))
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
