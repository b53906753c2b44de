#!/usr/bin/env python3
"""Paged KV-cache handoff: a prefill worker sends the blocks of one sequence
out of its block pool, a decode worker receives them into the (different)
blocks its own scheduler picked, in one message and without a gather copy
or a temporary on either side.

Both workers run in this process over a loopback connection; across two
processes on one node the same calls move the blocks over hipIpc / xGMI.
"""
import asyncio
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FULL = (1 << 64) - 1
BLOCKS, TOKENS, HEADS, DIM = 64, 16, 8, 128  # 32 KiB of fp16 per block


async def main() -> None:
    import torch

    import starway_amd as sw

    if not sw.gpu_available():
        sys.exit("paged_kv_handoff: needs a HIP device")
    prefill_pool = torch.randn(BLOCKS, TOKENS, HEADS, DIM, device="cuda",
                               dtype=torch.float16)
    decode_pool = torch.zeros_like(prefill_pool)
    # Block ids come from each side's scheduler, on the host.
    prefill_blocks = [7, 0, 31, 4]
    decode_blocks = [2, 9, 10, 5]
    torch.cuda.synchronize()

    server, client = sw.Server(), sw.Client()  # decode, prefill
    await client.aconnect_address(server.listen_address())

    fut = server.arecv(decode_pool, 1, FULL, index=decode_blocks)
    await client.asend(prefill_pool, 1, index=prefill_blocks)
    tag, length = await fut
    torch.cuda.synchronize()

    block_bytes = prefill_pool[0].numel() * prefill_pool.element_size()
    assert length == len(prefill_blocks) * block_bytes
    assert torch.equal(decode_pool[decode_blocks], prefill_pool[prefill_blocks])
    untouched = [b for b in range(BLOCKS) if b not in decode_blocks]
    assert decode_pool[untouched].eq(0).all()
    print(f"moved {len(prefill_blocks)} blocks ({length} B) "
          f"{prefill_blocks} -> {decode_blocks}; "
          f"index_tx={client._client.get_stats()['index_tx']} "
          f"index_rx={server._server.get_stats()['index_rx']}")

    await client.aclose()
    await server.aclose()


if __name__ == "__main__":
    asyncio.run(main())
