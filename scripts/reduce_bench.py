#!/usr/bin/env python
"""Reducing receive: the fused accumulate kernel against copy-then-add.

Same device, per size and dtype, the variants alternated round by round in
one process:

* ``fused``     _accum_sync with the default tuning (what a reducing
                receive launches)
* ``fused_plain`` / ``fused_nt``  (``--nt``) the bulk kernel forced to plain
                or to non-temporal source loads, whatever the size
* ``unfused``   _copy_device_sync into a temporary, then ``acc.add_(tmp)``
                -- what a user does today per message, both steps timed
* ``copy``      _copy_device_sync alone, for scale

Every call is timed on the host clock and ends in a device synchronise
(both hooks synchronise their stream; the add is followed by
torch.cuda.synchronize()). So ``unfused`` pays two launch-and-wait round
trips where ``fused`` pays one: that is the user-visible cost being
compared, and it is why the small sizes say little about the kernels.

Per variant: median over rounds of the mean time of ``--calls`` calls, the
spread (max - min over rounds, relative to the median), and GB/s of HBM
traffic by the traffic model (fused 3x payload: read source, read and write
the accumulator; unfused 5x; copy 2x). One JSON line per (size, dtype).

Needs a GPU; there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

NT_NEVER = 1 << 62
TRAFFIC = {"fused": 3, "fused_plain": 3, "fused_nt": 3, "unfused": 5,
           "copy": 2}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes-mib", type=int, nargs="+",
                    default=[1, 16, 64, 256])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nt", action="store_true",
                    help="also force plain / non-temporal source loads")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if args.rounds < 7 or args.calls < 10:
        ap.error("at least 7 rounds of 10 calls")

    import torch

    import starway_amd as sw
    from starway_amd import _core

    if not sw.gpu_available():
        print("reduce_bench: no HIP device", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    variants = ["fused", "unfused", "copy"] + (
        ["fused_plain", "fused_nt"] if args.nt else [])
    lines = []
    for dtype in args.dtypes:
        td = getattr(torch, dtype)
        for mib in args.sizes_mib:
            nbytes = mib << 20
            n = nbytes // torch.empty(0, dtype=td).element_size()
            acc = torch.rand(n, device="cuda").to(td)
            src = torch.rand(n, device="cuda").to(td)
            tmp = torch.empty_like(src)
            torch.cuda.synchronize()
            a, s, t = acc.data_ptr(), src.data_ptr(), tmp.data_ptr()

            def fused():
                _core._accum_sync(a, s, nbytes, dtype, 0)

            def fused_plain():
                _core._accum_sync(a, s, nbytes, dtype, 0,
                                  nt_threshold=NT_NEVER)

            def fused_nt():
                _core._accum_sync(a, s, nbytes, dtype, 0, nt_threshold=1)

            def unfused():
                _core._copy_device_sync(t, s, nbytes, 0)
                acc.add_(tmp)
                torch.cuda.synchronize()

            def copy():
                _core._copy_device_sync(t, s, nbytes, 0)

            fns = {"fused": fused, "fused_plain": fused_plain,
                   "fused_nt": fused_nt, "unfused": unfused, "copy": copy}
            for v in variants:
                for _ in range(args.warmup):
                    fns[v]()
            per_round = {v: [] for v in variants}
            for r in range(args.rounds):
                # Rotate the starting variant so none always runs first.
                order = variants[r % len(variants):] + \
                    variants[:r % len(variants)]
                for v in order:
                    fn = fns[v]
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn()
                    per_round[v].append(
                        (time.perf_counter() - t0) / args.calls)
            rec = {"dtype": dtype, "mib": mib, "rounds": args.rounds,
                   "calls": args.calls}
            for v in variants:
                med = statistics.median(per_round[v])
                rec[v] = {
                    "median_us": round(med * 1e6, 2),
                    "min_us": round(min(per_round[v]) * 1e6, 2),
                    "max_us": round(max(per_round[v]) * 1e6, 2),
                    "spread": round(
                        (max(per_round[v]) - min(per_round[v])) / med, 4),
                    "hbm_gbps": round(TRAFFIC[v] * nbytes / med / 1e9, 1),
                }
            rec["fused_over_unfused"] = round(
                rec["fused"]["median_us"] / rec["unfused"]["median_us"], 4)
            # Fused wins only if even its slowest round beats the unfused
            # variant's fastest one: a margin larger than both spreads.
            rec["fused_wins_beyond_spread"] = (
                rec["fused"]["max_us"] < rec["unfused"]["min_us"])
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del acc, src, tmp
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
