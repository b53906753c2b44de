#!/usr/bin/env python
"""Converting receive: the fused convert kernel against receive-then-cast.

Same-device loopback (one Server, one Client, one process), per direction
and message size, the variants alternated round by round:

* ``fused_a`` / ``fused_b``  a converting receive, ``arecv(buf, ...,
                msg_dtype=...)``, with lane shape "a" (8 elements per lane)
                or "b" (4) forced for the process through
                ``_core._convert_shape``
* ``baseline``  what a user does without it: a plain receive into a
                temporary of the message's dtype, then torch ``acc += tmp``
                (or ``buf.copy_(tmp)``), timed to the end of the torch op
* ``same_dtype``  for context, the existing receive at the same element
                count with a message of the buffer's own dtype
                (``reduce="sum"`` where the direction accumulates)

Directions: ``bf16_to_f32_sum`` (bf16 message added into an fp32
accumulator) and ``f32_to_bf16`` (fp32 message written into a bf16 buffer).
Sizes are bytes of MESSAGE.

Every call is one receive posted, one send, both awaited, and for the
baseline the torch op and a device synchronise on top. Per variant: median
over rounds of the mean time of ``--calls`` calls, the fastest and slowest
round, and GB/s of HBM traffic by the traffic model (per element, bf16 into
fp32: fused 2 + 4 + 4 B, baseline 2 + 2 then 2 + 4 + 4 B). One JSON line
per (direction, size).

One GPU shows nothing about a pull over xGMI: there the fused path also
halves the bytes on the link for a bf16 message, which stays reasoning
until it is measured on two.

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
VARIANTS = ["fused_a", "fused_b", "baseline", "same_dtype"]
# direction -> (message dtype, buffer dtype, accumulate)
DIRECTIONS = {
    "bf16_to_f32_sum": ("bfloat16", "float32", True),
    "f32_to_bf16": ("float32", "bfloat16", False),
}


def traffic_bytes(variant, n, ms, bs, acc):
    """HBM bytes one call moves, by the model in the module docstring."""
    rmw = 2 * bs if acc else bs          # the buffer: read+write, or write
    if variant in ("fused_a", "fused_b"):
        return n * (ms + rmw)
    if variant == "baseline":
        return n * (2 * ms + ms + rmw)
    return n * (bs + rmw)                # same_dtype


async def run(args) -> int:
    import torch

    import starway_amd as sw
    from starway_amd import _core

    if not sw.gpu_available():
        print("convert_bench: no HIP device", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    prod = _core._convert_shape()
    server, client = sw.Server(), sw.Client()
    await client.aconnect_address(server.listen_address())
    lines = []
    try:
        for name in args.directions:
            msg_dtype, buf_dtype, acc = DIRECTIONS[name]
            mt, bt = getattr(torch, msg_dtype), getattr(torch, buf_dtype)
            ms = torch.empty(0, dtype=mt).element_size()
            bs = torch.empty(0, dtype=bt).element_size()
            reduce = "sum" if acc else None
            for mib in args.sizes_mib:
                n = (mib << 20) // ms
                msg = torch.rand(n, device="cuda").to(mt)
                same = torch.rand(n, device="cuda").to(bt)
                buf = torch.rand(n, device="cuda").to(bt)
                tmp = torch.empty_like(msg)
                torch.cuda.synchronize()

                async def deliver(dst, src, **kw):
                    fut = server.arecv(dst, 1, FULL, **kw)
                    await client.asend(src, 1)
                    await fut

                async def fused():
                    await deliver(buf, msg, reduce=reduce, msg_dtype=mt)

                async def baseline():
                    await deliver(tmp, msg)
                    if acc:
                        buf.add_(tmp)
                    else:
                        buf.copy_(tmp)
                    torch.cuda.synchronize()

                async def same_dtype():
                    await deliver(buf, same, reduce=reduce)

                async def call(v):
                    if v.startswith("fused_"):
                        _core._convert_shape(v[-1])
                        await fused()
                    elif v == "baseline":
                        await baseline()
                    else:
                        await same_dtype()

                for v in VARIANTS:
                    for _ in range(args.warmup):
                        await call(v)
                per_round = {v: [] for v in VARIANTS}
                for r in range(args.rounds):
                    # Rotate the starting variant so none always runs first.
                    k = r % len(VARIANTS)
                    for v in VARIANTS[k:] + VARIANTS[:k]:
                        t0 = time.perf_counter()
                        for _ in range(args.calls):
                            await call(v)
                        per_round[v].append(
                            (time.perf_counter() - t0) / args.calls)
                rec = {"direction": name, "msg_mib": mib, "elements": n,
                       "rounds": args.rounds, "calls": args.calls,
                       "production_shape": prod, "gpus": 1}
                for v in VARIANTS:
                    med = statistics.median(per_round[v])
                    rec[v] = {
                        "median_us": round(med * 1e6, 2),
                        "min_us": round(min(per_round[v]) * 1e6, 2),
                        "max_us": round(max(per_round[v]) * 1e6, 2),
                        "hbm_gbps": round(
                            traffic_bytes(v, n, ms, bs, acc) / med / 1e9, 1),
                    }
                fused_prod = rec["fused_" + prod]
                rec["fused_over_baseline"] = round(
                    fused_prod["median_us"] / rec["baseline"]["median_us"], 4)
                # The production shape wins only if even its slowest round
                # beats the baseline's fastest one: the ranges do not overlap.
                rec["fused_wins_beyond_spread"] = (
                    fused_prod["max_us"] < rec["baseline"]["min_us"])
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
                del msg, same, buf, tmp
    finally:
        _core._convert_shape("")
        await client.aclose()
        await server.aclose()
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes-mib", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--directions", nargs="+", default=list(DIRECTIONS),
                    choices=list(DIRECTIONS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if args.rounds < 7 or args.calls < 10:
        ap.error("at least 7 rounds of 10 calls")
    return asyncio.run(run(args))


if __name__ == "__main__":
    sys.exit(main())
