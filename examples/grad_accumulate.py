#!/usr/bin/env python3
"""Mixed-precision gradient accumulation: N workers each send a bf16
gradient, the server sums them into an fp32 accumulator inside the pull
kernel -- no bf16 temporary, no second pass, and every contribution is added
in fp32 and rounded once.

All endpoints run in this process over loopback connections; across
processes on one node the same calls pull the bf16 bytes over hipIpc /
xGMI, 2 B per element on the link where an fp32 message would move 4.
"""
import asyncio
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

WORKERS, ELEMS = 8, 1 << 20


async def main() -> None:
    import torch

    import starway_amd as sw

    if not sw.gpu_available():
        sys.exit("grad_accumulate: needs a HIP device")
    grads = [torch.randn(ELEMS, device="cuda").to(torch.bfloat16)
             for _ in range(WORKERS)]
    acc = torch.full((ELEMS,), 256.0, device="cuda")  # fp32 master copy
    acc_bf16 = acc.to(torch.bfloat16)                 # what bf16 would give
    expected = acc.clone()
    for g in grads:
        expected += g.float()
        acc_bf16 = (acc_bf16.float() + g.float()).to(torch.bfloat16)
    torch.cuda.synchronize()

    server = sw.Server()
    workers = [sw.Client() for _ in range(WORKERS)]
    addr = server.listen_address()
    for w in workers:
        await w.aconnect_address(addr)

    # Any number of reducing receives may be outstanding on one buffer.
    futs = [server.arecv(acc, 0, 0, reduce="sum", msg_dtype=torch.bfloat16)
            for _ in range(WORKERS)]
    await asyncio.gather(*[w.asend(g, rank)
                           for rank, (w, g) in enumerate(zip(workers, grads))])
    lengths = [(await f)[1] for f in futs]
    torch.cuda.synchronize()

    assert lengths == [2 * ELEMS] * WORKERS  # bytes of message, bf16
    # fp32 sums of the same values in another order: equal to rounding.
    assert torch.allclose(acc, expected, rtol=0, atol=1e-3)
    drift = (acc_bf16.float() - expected).abs().max().item()
    stats = server._server.get_stats()
    print(f"summed {WORKERS} bf16 gradients of {ELEMS} elements into fp32; "
          f"max error {(acc - expected).abs().max().item():.2e} "
          f"(a bf16 accumulator would be off by {drift:.2f}); "
          f"cast_rx={stats['cast_rx']} reduce_rx={stats['reduce_rx']}")

    for w in workers:
        await w.aclose()
    await server.aclose()


if __name__ == "__main__":
    asyncio.run(main())
