#!/usr/bin/env python3
"""Copy-kernel microbench: bandwidth per size through sw::k_copy_b128<U, NT>.

Used under rocprofv3 for kernel-trace/PMC evidence:
  rocprofv3 --kernel-trace --stats -d out -- python scripts/kernel_bench.py
  rocprofv3 --pmc FETCH_SIZE WRITE_SIZE --kernel-trace -d out -- \
      python scripts/kernel_bench.py --sizes 268435456

--nd times the N-D pack kernels instead (docs/benchmark.md "N-D layouts"):
a strided fp16 view packed into a contiguous buffer, per shape and size
  generic     k_copy_nd          (_copy_nd_sync path="generic")
  tiled       k_copy_nd_tile     (path="tiled", transpose family only)
  contiguous  torch .contiguous() into a temporary, then the flat copy:
              what a caller had to do before N-D layouts were accepted
  flat        the flat copy of the same byte count (the ceiling)
Every variant is warmed, the variants alternate within each round, and the
spread over the rounds is printed next to the median. A call is timed with
the host clock around work that ends in a stream synchronise.
"""
from __future__ import annotations

import os

# ROCm multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues
# (default 4); oversubscription time-slices co-mapped streams at ~ms
# granularity. Must be set before the FIRST HIP init in the process
# (torch's or ours) — see ROUND2_NOTES.md "hardware-queue starvation".
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def nd_views(torch, mib: int):
    """name -> strided fp16 view holding `mib` MiB."""
    n = mib << 19  # fp16 elements
    rows = 4096 if mib <= 64 else 8192
    b = n // (16 * 4096 * 128)
    return {
        # (rows, n/rows) stored as its transpose.
        "transpose2d": torch.empty(n // rows, rows, dtype=torch.float16,
                                   device="cuda").normal_().t(),
        # (B,H,S,D) -> (B,S,H,D), D=128: dense runs of 256 B.
        "bhsd_to_bshd": torch.empty(b, 16, 4096, 128, dtype=torch.float16,
                                    device="cuda").normal_()
                             .permute(0, 2, 1, 3),
    }


def bench_nd(args) -> None:
    import json
    import statistics

    import torch

    from starway_amd import _core

    torch.cuda.set_device(0)
    results = []
    for mib in args.nd_mib:
        for name, view in nd_views(torch, mib).items():
            es = view.element_size()
            nbytes = view.numel() * es
            dst = torch.empty(view.numel(), dtype=view.dtype, device="cuda")
            flat_src = torch.empty_like(dst).normal_()
            shape = list(view.shape)
            strides = [s * es for s in view.stride()]
            dense = [s * es for s in view.contiguous().stride()]
            torch.cuda.synchronize()

            def nd(path):
                _core._copy_nd_sync(dst.data_ptr(), shape, dense,
                                    view.data_ptr(), shape, strides, es, 0,
                                    path=path)

            def via_contiguous():
                tmp = view.contiguous()
                torch.cuda.synchronize()
                _core._copy_device_sync(dst.data_ptr(), tmp.data_ptr(),
                                        nbytes, 0)

            def flat():
                _core._copy_device_sync(dst.data_ptr(), flat_src.data_ptr(),
                                        nbytes, 0)

            variants = {"generic": lambda: nd("generic")}
            try:
                nd("tiled")
                variants["tiled"] = lambda: nd("tiled")
            except ValueError:
                pass  # not in the transpose family
            variants["contiguous"] = via_contiguous
            variants["flat"] = flat
            want = view.contiguous().reshape(-1)
            for vname, fn in variants.items():  # warm-up + correctness
                dst.zero_()
                torch.cuda.synchronize()  # the hooks run on their own stream
                fn()
                if vname != "flat":
                    assert torch.equal(dst, want), f"{name} {vname} mismatch"
            times = {v: [] for v in variants}
            for _ in range(args.rounds):
                for vname, fn in variants.items():
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        fn()
                    times[vname].append(
                        (time.perf_counter() - t0) / args.iters)
            for vname, ts in times.items():
                med = statistics.median(ts)
                row = {"shape": name, "mib": mib, "variant": vname,
                       "median_us": med * 1e6, "min_us": min(ts) * 1e6,
                       "max_us": max(ts) * 1e6,
                       "payload_gbps": nbytes / med / 1e9}
                results.append(row)
                print(f"{name:>13} {mib:>4} MiB {vname:>10}: "
                      f"{row['median_us']:9.1f} us median "
                      f"[{row['min_us']:.1f} .. {row['max_us']:.1f}] "
                      f"{row['payload_gbps']:8.1f} GB/s payload", flush=True)
            del dst, flat_src, view
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nd", action="store_true",
                    help="time the N-D pack kernels (see module docstring)")
    ap.add_argument("--nd-mib", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", help="--nd: also write the rows as JSON here")
    ap.add_argument("--sizes", type=int, nargs="*",
                    default=[1 << 20, 16 << 20, 256 << 20, 1 << 30])
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if args.nd:
        bench_nd(args)
        return

    import torch

    from starway_amd import _core

    torch.cuda.set_device(0)
    for size in args.sizes:
        src = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        torch.cuda.synchronize()
        # warmup + correctness
        _core._copy_device_sync(dst.data_ptr(), src.data_ptr(), size, 0)
        assert torch.equal(src, dst), "copy kernel mismatch"
        t0 = time.perf_counter()
        for _ in range(args.iters):
            _core._copy_device_sync(dst.data_ptr(), src.data_ptr(), size, 0)
        dt = (time.perf_counter() - t0) / args.iters
        print(f"{size:>12} B: {size / dt / 1e12:.3f} TB/s payload "
              f"({2 * size / dt / 1e12:.3f} TB/s HBM traffic), {dt * 1e6:.1f} us",
              flush=True)


if __name__ == "__main__":
    main()
