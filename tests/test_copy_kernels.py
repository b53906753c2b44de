"""Direct, guard-banded, byte-exact tests of every copy kernel in
csrc/kernels.hip and every branch of its host-side dispatch.

Each case runs through tests/_guard.py: seeded CPU bytes are the reference,
the destination arena is prefilled so an unwritten byte cannot match, and
the whole arena (guards and inter-row gaps included) is compared with a
numpy expectation. No tolerances.

The launch tuning is passed explicitly (block_cap / nt_threshold /
nt_unroll), so one process reaches the capped-grid multi-iteration loops
and all three 16 B kernels at sizes of a few tens of KiB:

  block_cap=2  ->  2 blocks x 256 threads: grid stride 512 elements of 16 B,
                   one x4-unrolled pass = 2048 elements (32 KiB),
                   one x8-unrolled pass = 4096 elements (64 KiB).
"""
import itertools

import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from starway_amd import _core  # noqa: E402

from _guard import GuardedCopy, Region  # noqa: E402

HUGE = 1 << 62  # nt_threshold that no message reaches: plain loads and stores

# kernel id -> (nt_threshold, nt_unroll). The ids are the kernels' former
# names: k_copy_b128<4, false>, <4, true> and <8, true>.
KERNELS = {
    "k_copy_b128": (HUGE, 4),
    "k_copy_b128_nt": (1, 4),
    "k_copy_b128_nt_u8": (1, 8),
}

# n16 (count of 16 B bulk elements) -> what it reaches at block_cap=2. The
# grid is sized from n16/4+1 work items (n16/8+1 for the x8 kernel), so it
# is one block (stride 256) below n16=1020 (2040 for x8) and the capped two
# blocks (stride 512) from there on.
N16_X4 = [
    1,              # one lane, remainder loop only
    255, 256,       # one block, partial / full single stride
    511, 512, 513,  # one block: remainder loop twice per lane, 513 wraps a
                    # third time on lane 0 (x8 kernel: same, no full pass)
    2047,           # stride 512: lanes 0..510 take one x4 pass, lane 511
                    # takes the remainder loop three times instead
    2048,           # exactly one x4 pass on every lane, no remainder
    2049,           # one x4 pass + 1 remainder element (lane 0)
    3 * 2048 + 5,   # three x4 passes + 5 remainder elements
    2048 + 1535,    # one x4 pass + a remainder of up to three strides
]
N16_X8_EXTRA = [
    4095,           # lanes 0..510 take one x8 pass, lane 511 the remainder
    4096,           # exactly one x8 pass on every lane
    4097,           # one x8 pass + 1 remainder element (lane 0)
    2 * 4096 + 513,  # two x8 passes + a remainder that wraps once
]

OFFSETS = [0, 1, 15]
TAILS = [0, 1, 15]


def _run_flat(seed, src_off, dst_off, nbytes, label, **tuning):
    case = GuardedCopy(seed, Region.flat(src_off, nbytes),
                       Region.flat(dst_off, nbytes))
    _core._copy_device_sync(case.dst_ptr, case.src_ptr, nbytes, 0, **tuning)
    case.check(label)


def _kernel_cases():
    for name in KERNELS:
        sizes = N16_X4 + (N16_X8_EXTRA if name.endswith("_u8") else [])
        for n16 in sizes:
            yield pytest.param(name, n16, id=f"{name}-n16_{n16}")


# =============================================================================
# Contiguous, co-aligned: head (k_copy_elem<1>) + 16 B bulk + tail (same)
# =============================================================================


@pytest.mark.parametrize("kernel,n16", list(_kernel_cases()))
def test_coaligned_capped_grid(kernel, n16):
    """block_cap=2: the grid-stride loops run several iterations per lane.
    Every bulk size is crossed with byte offsets {0,1,15} (head of 0, 15,
    1 bytes) and byte tails {0,1,15}."""
    nt_threshold, nt_unroll = KERNELS[kernel]
    for k, (off, tail) in enumerate(itertools.product(OFFSETS, TAILS)):
        head = (16 - off) % 16
        nbytes = head + n16 * 16 + tail
        _run_flat(1000 + n16 * 16 + k, off, off, nbytes,
                  f"{kernel} n16={n16} off={off} tail={tail}",
                  block_cap=2, nt_threshold=nt_threshold,
                  nt_unroll=nt_unroll)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_coaligned_single_block(kernel):
    """block_cap=1: one block walks the whole message (stride 256)."""
    nt_threshold, nt_unroll = KERNELS[kernel]
    # 256*8*2 + 256*3 + 7 elements: two x8 passes (four x4 passes) plus a
    # remainder of three strides and a partial one; odd head and tail.
    n16 = 256 * 8 * 2 + 256 * 3 + 7
    _run_flat(2000, 9, 9, 7 + n16 * 16 + 5, f"{kernel} cap=1",
              block_cap=1, nt_threshold=nt_threshold, nt_unroll=nt_unroll)


@pytest.mark.parametrize("nbytes", [1, 3])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_coaligned_head_only(kernel, nbytes):
    """Offset 13 wants a 3-byte head: nbytes=1 clips it (head > bytes),
    nbytes=3 is all head. No bulk and no tail launch may follow."""
    nt_threshold, nt_unroll = KERNELS[kernel]
    _run_flat(2100 + nbytes, 13, 13, nbytes, f"{kernel} head-only",
              block_cap=2, nt_threshold=nt_threshold, nt_unroll=nt_unroll)


def test_default_tuning_capped_grid_nt():
    """Default tuning at the smallest size that caps the default grid
    (8192 blocks): the non-temporal x4 kernel with a wrapped grid and a
    remainder loop -- the configuration bench.py's default message runs."""
    t = _core._copy_tuning()
    nbytes = (128 << 20) + (64 << 10) + 21
    n16 = (nbytes - 11) // 16  # offset 5: 11-byte head
    if (t["block_cap"], t["nt_threshold"], t["nt_unroll"]) == (
            8192, 64 << 20, 4):
        # n16/4+1 work items want more than 8192 blocks: the grid is capped
        # and each lane runs one x4 pass plus the remainder loop.
        assert (n16 // 4 + 1 + 255) // 256 > t["block_cap"]
        assert nbytes >= t["nt_threshold"]
    _run_flat(2200, 5, 5, nbytes, "default tuning 128 MiB + 64 KiB + 21")


# =============================================================================
# Contiguous, src and dst not co-aligned: k_copy_elem<4> / full-grid <1>
# =============================================================================

MISALIGNED_SIZES = [1, 4, 1023, 1024, 40_000]
DWORD_OFFSETS = [(0, 4), (4, 8), (12, 0)]
BYTE_OFFSETS = [(1, 2), (3, 0), (0, 15)]


@pytest.mark.parametrize("offs", DWORD_OFFSETS,
                         ids=lambda o: f"src{o[0]}_dst{o[1]}")
@pytest.mark.parametrize("nbytes", [n for n in MISALIGNED_SIZES if n % 4 == 0])
def test_k_copy_b32_dword_coaligned(offs, nbytes):
    """4 B-co-aligned pointers, size a multiple of 4: the dword kernel.
    40 000 B at block_cap=2 is 10 000 dwords over a 512-lane grid."""
    _run_flat(3000 + nbytes + offs[1], offs[0], offs[1], nbytes,
              f"k_copy_elem<4> {offs}", block_cap=2)


@pytest.mark.parametrize(
    "offs,nbytes",
    [(o, n) for o in DWORD_OFFSETS for n in MISALIGNED_SIZES if n % 4]
    + [(o, n) for o in BYTE_OFFSETS for n in MISALIGNED_SIZES],
    ids=lambda v: f"src{v[0]}_dst{v[1]}" if isinstance(v, tuple) else str(v))
def test_k_copy_b8_full_grid(offs, nbytes):
    """Neither 16 B- nor dword-copyable: the byte kernel over a full grid
    (40 000 B at block_cap=2: 79 iterations per lane)."""
    _run_flat(3100 + nbytes + 16 * offs[0] + offs[1], offs[0], offs[1],
              nbytes, f"k_copy_elem<1> {offs}", block_cap=2)


@pytest.mark.parametrize("offs", [(0, 0), (5, 5), (0, 4), (1, 2)],
                         ids=lambda o: f"src{o[0]}_dst{o[1]}")
def test_zero_bytes_is_a_noop(offs):
    # Valid pointers inside the arenas; nothing may be written.
    _run_flat(3200, offs[0], offs[1], 0, "nbytes=0", block_cap=2)


# =============================================================================
# Strided: k_copy_strided<16> (vec) / k_copy_strided<1>
# =============================================================================


def _run_strided(seed, src: Region, dst: Region, label, block_cap=0):
    case = GuardedCopy(seed, src, dst)
    _core._copy_strided_sync(case.dst_ptr, dst.stride, case.src_ptr,
                             src.stride, src.rows, src.row_bytes, 0,
                             block_cap)
    case.check(label)


# (src_stride - row_bytes, dst_stride - row_bytes)
VEC_LAYOUTS = {
    "sstride_lt_dstride": (16, 112),
    "dense_src": (0, 112),
    "dense_dst": (16, 0),
}


@pytest.mark.parametrize("block_cap", [0, 1], ids=["cap_default", "cap_1"])
@pytest.mark.parametrize("layout", list(VEC_LAYOUTS))
@pytest.mark.parametrize("row_bytes", [16, 48, 1040])
@pytest.mark.parametrize("rows", [1, 2, 3, 67])
def test_k_copy_strided_b128(rows, row_bytes, layout, block_cap):
    """All five `vec` conditions hold. Strides differ between the sides;
    each side is also dense once. 67 x 1040 B at block_cap=1 is 4355
    elements over 256 lanes (18 iterations, rows change mid-stride)."""
    ss, ds = (row_bytes + pad for pad in VEC_LAYOUTS[layout])
    _run_strided(4000 + rows * 7 + row_bytes,
                 Region(0, rows, row_bytes, ss),
                 Region(0, rows, row_bytes, ds),
                 f"k_copy_strided<16> rows={rows} rb={row_bytes} "
                 f"sstride={ss} dstride={ds} cap={block_cap}", block_cap)


@pytest.mark.parametrize("block_cap", [0, 1], ids=["cap_default", "cap_1"])
@pytest.mark.parametrize("row_bytes", [1, 17, 255])
@pytest.mark.parametrize("rows", [1, 2, 3, 67])
def test_k_copy_strided_b8(rows, row_bytes, block_cap):
    """Odd row lengths, odd strides, pointer offsets 1 and 7."""
    ss, ds = (row_bytes + 2) | 1, (row_bytes + 6) | 1
    for k, (so, do) in enumerate([(1, 7), (7, 1), (1, 1)]):
        _run_strided(4100 + rows * 7 + row_bytes + k,
                     Region(so, rows, row_bytes, ss),
                     Region(do, rows, row_bytes, ds),
                     f"k_copy_strided<1> rows={rows} rb={row_bytes} "
                     f"src+{so} dst+{do} cap={block_cap}", block_cap)


# Exactly one `vec` condition false, the other four 16-aligned:
# (src_off, dst_off, src_stride, dst_stride, row_bytes)
ONE_FALSE = {
    "src_ptr": (4, 0, 64, 80, 48),
    "dst_ptr": (0, 8, 64, 80, 48),
    "src_stride": (0, 0, 68, 80, 48),
    "dst_stride": (0, 0, 64, 84, 48),
    "row_bytes": (0, 0, 64, 80, 40),
}


@pytest.mark.parametrize("which", list(ONE_FALSE))
def test_strided_one_vec_condition_false(which):
    """Each condition of launch_copy_strided's `vec` predicate failing
    alone must send the copy down the byte kernel, still exact."""
    so, do, ss, ds, rb = ONE_FALSE[which]
    misaligned = [so % 16 != 0, do % 16 != 0, ss % 16 != 0, ds % 16 != 0,
                  rb % 16 != 0]
    assert sum(misaligned) == 1
    for block_cap in (0, 1):
        _run_strided(4200 + len(which), Region(so, 5, rb, ss),
                     Region(do, 5, rb, ds),
                     f"k_copy_strided<1> via {which} cap={block_cap}",
                     block_cap)


@pytest.mark.parametrize("rows,row_bytes", [(0, 48), (5, 0), (0, 0)])
def test_strided_empty_is_a_noop(rows, row_bytes):
    _run_strided(4300, Region(0, rows, row_bytes, 64),
                 Region(0, rows, row_bytes, 80), "strided no-op")


# =============================================================================
# Multi: k_copy_multi, one block per descriptor
# =============================================================================

# (nbytes, src_off, dst_off): sizes and alignments mixed within one launch.
MULTI_SPECS = [
    (4096, 0, 0),      # aligned, %16 == 0: vector branch
    (4097, 0, 0),      # aligned pointers, odd size: byte branch
    (16, 1, 0),        # src-only misaligned
    (65536, 0, 3),     # dst-only misaligned, 256 iterations per lane
    (0, 0, 0),         # empty descriptor: block writes nothing
    (1, 0, 0),
    (4096 + 16, 0, 0),  # vector branch, 257 elements: lane 0 wraps
    (65536, 0, 0),     # vector branch, 16 iterations per lane
]


# The block copy's edge sizes through both of its branches (16 B vectors:
# both pointers and the size multiples of 16; bytes: anything else), and a
# 4 KiB message with either pointer one byte off 16 B alignment.
MULTI_EDGE_SPECS = [
    (16, 0, 0),        # one 16 B element: vector branch
    (0, 1, 0),         # empty through the byte branch
    (15, 0, 0),
    (17, 0, 0),
    (16, 0, 1),        # dst-only misaligned, a single element's worth
    (4096, 1, 0),
    (4096, 0, 1),
]


def _run_multi(specs, label):
    cases = [GuardedCopy(5000 + 31 * i + n, Region.flat(so, n),
                         Region.flat(do, n))
             for i, (n, so, do) in enumerate(specs)]
    _core._copy_multi_sync(
        [(c.dst_ptr, c.src_ptr, c.src.nbytes) for c in cases], 0)
    for i, c in enumerate(cases):
        c.check(f"{label} desc {i} {specs[i]}")


@pytest.mark.parametrize("n", [1, 3, 8])
def test_k_copy_multi(n):
    if n == 1:
        for spec in MULTI_SPECS + MULTI_EDGE_SPECS:  # every kind alone
            _run_multi([spec], "k_copy_multi n=1")
    else:
        _run_multi(MULTI_SPECS[:n], f"k_copy_multi n={n}")
        # Rotated, so other kinds occupy block 0 and the last block.
        _run_multi(MULTI_SPECS[-n:][::-1], f"k_copy_multi n={n} reversed")


@pytest.mark.parametrize("n", [0, 9])
def test_copy_multi_rejects_bad_batch(n):
    case = GuardedCopy(5100, Region.flat(0, 16), Region.flat(0, 16))
    with pytest.raises(ValueError):
        _core._copy_multi_sync([(case.dst_ptr, case.src_ptr, 16)] * n, 0)
    # Rejected before any launch: the destination keeps its prefill.
    assert (case.dst_buf.cpu().numpy() == case.dst_host).all()


def test_copy_multi_rejects_oversize_descriptor():
    case = GuardedCopy(5101, Region.flat(0, 16), Region.flat(0, 16))
    with pytest.raises(ValueError):
        _core._copy_multi_sync([(case.dst_ptr, case.src_ptr, 1 << 32)], 0)
    assert (case.dst_buf.cpu().numpy() == case.dst_host).all()
