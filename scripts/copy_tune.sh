#!/bin/bash
# On-box copy-kernel sweep with bin/copy_bench, raw per-round output on
# stdout (redirect it into profiles/).
#
#  1. Streaming kernel family (csrc/copy_stream.hpp) against the grid-stride
#     kernels, alternating round by round inside one process:
#     sizes 64 MiB / 128 MiB / 256 MiB / 1 GiB x stream_blocks
#     1024 / 2048 / 8192 / uncapped x every instantiation, ROUNDS rounds.
#  2. The older axes of the grid-stride kernels: block cap x unroll at
#     256 MiB / 1 GiB.
#
# Every GPU step runs under its own time limit and the sweep stops at the
# first step that fails, so nothing more is started on the GPU after a
# fault or a hang.
cd "$(dirname "$0")/.." || exit 1
ROUNDS=${ROUNDS:-7}
ITERS=${ITERS:-20}
UNCAPPED=2147483647

step() {
  timeout -k 10 "$@"
  local rc=$?
  if [ $rc -ne 0 ]; then
    echo "step failed (exit $rc): $*" >&2
    exit $rc
  fi
}

for SZ in 67108864 134217728 268435456 1073741824; do
  for SB in 1024 2048 8192 $UNCAPPED; do
    echo "# size=$SZ stream_blocks=$SB rounds=$ROUNDS iters=$ITERS"
    step 180 ./bin/copy_bench --size $SZ --iters $ITERS --rounds $ROUNDS \
      --stream-blocks $SB --variants all
  done
done

for SZ in 268435456 1073741824; do
  for BLK in 2048 4096 8192 16384; do
    echo "# size=$SZ STARWAY_COPY_BLOCKS=$BLK rounds=$ROUNDS iters=$ITERS"
    STARWAY_COPY_BLOCKS=$BLK step 120 ./bin/copy_bench --size $SZ \
      --iters $ITERS --rounds $ROUNDS --variants old_nt4,old_nt8
  done
done
