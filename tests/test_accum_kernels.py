"""Bit-exact, guard-banded tests of the accumulate kernels (k_accum_b128,
k_accum_elem) and their dispatch (launch_accum), through the
synchronous hook ``_core._accum_sync``.

Sizes are derived from the kernels' shape, as in tests/test_copy_kernels.py:
256-thread workgroups, 16 B per lane, a x4-unrolled grid-stride loop. With
``block_cap=2`` the grid stride is 512 vectors and one unrolled iteration
covers 2048, so the bulk counts below sit on and around every boundary of
the grid, the unroll and the remainder loop at a few KiB.

Expectation, inputs and the whole-arena verdict: tests/_guard_accum.py.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from starway_amd import _core  # noqa: E402

DTYPE_NAMES = ["float32", "float16", "bfloat16", "int32"]
ES = {"float32": 4, "float16": 2, "bfloat16": 2, "int32": 4}
N16 = [1, 255, 256, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 + 5]
# Never reached by a message: the bulk kernel with plain source loads.
NT_NEVER = 1 << 62


def _run(case, *, block_cap, nt_threshold=NT_NEVER):
    _core._accum_sync(case.dst_ptr, case.src_ptr, case.nbytes, case.dtype, 0,
                      block_cap=block_cap, nt_threshold=nt_threshold)


def _case(seed, dtype, nbytes, src_off=0, dst_off=0):
    from _guard_accum import GuardedAccum

    return GuardedAccum(seed, dtype, nbytes, src_off=src_off, dst_off=dst_off)


@pytest.mark.parametrize("nt_threshold", [NT_NEVER, 1],
                         ids=["plain-src", "nt-src"])
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_coaligned_bulk_boundaries(dtype, nt_threshold):
    """Head, vector bulk and tail: every bulk count crossed with every
    element-aligned offset and tail."""
    es = ES[dtype]
    seed = 90_000
    for n16 in N16:
        for off in [0, es, 16 - es]:
            for tail in [0, es, 16 - es]:
                head = (16 - off) % 16
                nbytes = head + 16 * n16 + tail
                seed += 1
                case = _case(seed, dtype, nbytes, src_off=off, dst_off=off)
                _run(case, block_cap=2, nt_threshold=nt_threshold)
                case.check(f"{dtype} n16={n16} off={off} tail={tail}")


@pytest.mark.parametrize("nt_threshold", [NT_NEVER, 1],
                         ids=["plain-src", "nt-src"])
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_single_block_many_iterations(dtype, nt_threshold):
    """block_cap=1: two unrolled iterations, three remainder ones and a
    ragged end, all by one workgroup."""
    es = ES[dtype]
    n16 = 256 * 8 * 2 + 256 * 3 + 7
    off = 16 - es
    nbytes = es + 16 * n16 + es
    case = _case(91_000, dtype, nbytes, src_off=off, dst_off=off)
    _run(case, block_cap=1, nt_threshold=nt_threshold)
    case.check(f"{dtype} block_cap=1")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_sums_are_exact_on_both_sides_of_an_nt_threshold(dtype):
    """A correctness check at three sizes, no more: one vector below, at
    and above a threshold given to the hook. Both source-load variants give
    the same sums, so this cannot tell which of them ran or where the
    switch sits; each variant is forced through every bulk case above."""
    threshold = 16 * 600
    for k, n16 in enumerate([599, 600, 601]):
        case = _case(91_500 + k, dtype, 16 * n16)
        _run(case, block_cap=2, nt_threshold=threshold)
        case.check(f"{dtype} n16={n16} with nt_threshold={threshold}")


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_head_only(dtype):
    """A message that ends before the first 16 B boundary: the element
    kernel alone, one element."""
    es = ES[dtype]
    for k, off in enumerate([16 - es, 8]):
        case = _case(92_000 + k, dtype, es, src_off=off, dst_off=off)
        _run(case, block_cap=2)
        case.check(f"{dtype} head only at offset {off}")


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_not_coaligned_takes_the_element_kernel(dtype):
    es = ES[dtype]
    seed = 93_000
    for src_off, dst_off in [(0, es), (es, 0), (8, 0)]:
        for count in [1, 255, 256, 257, 2 * 512 + 3]:
            seed += 1
            case = _case(seed, dtype, count * es, src_off=src_off,
                         dst_off=dst_off)
            _run(case, block_cap=2)
            case.check(f"{dtype} src+{src_off} dst+{dst_off} n={count}")


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_zero_bytes_is_a_noop(dtype):
    case = _case(94_000, dtype, 0, src_off=ES[dtype])
    _run(case, block_cap=2)
    case.check_untouched(f"{dtype} zero bytes")


def test_default_tuning():
    """The process-default grid and threshold (what production launches)."""
    dtype = "float32"
    case = _case(95_000, dtype, 4 + 16 * 4099 + 8, src_off=12, dst_off=12)
    _core._accum_sync(case.dst_ptr, case.src_ptr, case.nbytes, dtype, 0)
    case.check("default tuning")
