"""The copy and accumulate kernels of csrc/kernels.hip at byte offsets past
2**31 and 2**32 from the pointer they are given, and the 64-bit index
instantiations of k_copy_nd and k_copy_indexed at their real size.

Far offsets, few bytes: the cases of the first half touch a few KiB spread
over two arenas of 6.25 GiB each (tests/_guard_far.py: numpy expectation,
every byte outside the touched windows must keep its constant, wrong
addresses of a kernel with narrowed offset arithmetic land inside the
allocation and fail a comparison). "Far" below means that the side's
offsets pass both 2**31 and 2**32; every case asserts that. Each case runs
with the default grid and with block_cap=1.

Whole messages past 4 GiB: the second half moves more than 2**32 bytes (or
granules) in one launch. Data is generated and verified on the device with
torch; the reference is torch's own indexing, .contiguous(), == and +,
never the code under test.

The module needs 32 GiB of free device memory (about 22 GiB at its peak)
and skips as a whole below that.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from starway_amd import _core  # noqa: E402

from _guard_far import (BODY, CHUNK, GUARD, NEED_FREE, P, FarArenas,  # noqa: E402
                        GuardedFar, Pool, View, aliases_of, dense)

CAPS = [0, 1]
MIB = 1 << 20
GIB = 1 << 30
NEVER = 1 << 62


@pytest.fixture(scope="module")
def arenas():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"far arenas need {NEED_FREE >> 30} GiB of free device "
                    f"memory, {free >> 30} GiB are free")
    a = FarArenas()
    yield a
    a.src.buf = a.dst.buf = None
    torch.cuda.empty_cache()


def far_case(arenas, seed, src, dst, far) -> GuardedFar:
    """`far` names the sides ("s", "d") whose offsets must pass 2**31 and
    2**32; the other side must stay below 2**31."""
    case = GuardedFar(arenas, seed, src, dst)
    for tag, side in (("s", src), ("d", dst)):
        if tag in far:
            assert case.crosses(side), f"{side} is not far"
        else:
            assert case.rel_offsets(side).max() < 2 ** 31, f"{side} not near"
    return case


# =============================================================================
# k_copy_indexed at far offsets
# =============================================================================

ENTRIES = (4100, 0, 2050, 4099, 3)
SIX = (4100, 0, 2050, 4099, 3, 2049)
FOUR = (4099, 0, 2051, 4100)


def pool(slice_bytes, pitch, index=ENTRIES, off=0) -> Pool:
    return Pool(off, max(index) + 1, slice_bytes, pitch, index)


def gather_scatter(label, p: Pool):
    return [(f"{label}, gather", p, dense(0, p.nbytes), "s"),
            (f"{label}, scatter", dense(0, p.nbytes), p, "d")]


# Both factors of index * stride fit 32 bits, the product does not.
BIG_INDEX = (4_150_000, 0, 2_070_000, 4_149_999)
assert max(BIG_INDEX) < 2 ** 32 and max(BIG_INDEX) * 1040 >= 2 ** 32

INDEXED = [
    *gather_scatter("16 B, pitch 2**20 + 16", pool(1040, 2 ** 20 + 16)),
    ("16 B, indexed -> indexed, boundaries interleave",
     pool(768, 2 ** 20 + 16, SIX), pool(1152, 2 ** 20 + 16, FOUR, 16), "sd"),
    *gather_scatter("4 B, pitch 2**20 + 4", pool(1044, 2 ** 20 + 4)),
    ("4 B, indexed -> indexed", pool(776, 2 ** 20 + 4, SIX),
     pool(1164, 2 ** 20 + 4, FOUR, 4), "sd"),
    *gather_scatter("1 B, pitch 2**20 + 3", pool(1041, 2 ** 20 + 3)),
    ("1 B, indexed -> indexed", pool(770, 2 ** 20 + 3, SIX),
     pool(1155, 2 ** 20 + 3, FOUR, 1), "sd"),
    *gather_scatter("large index, pitch 1040, no gap",
                    pool(1040, 1040, BIG_INDEX)),
]


def run_indexed(arenas, k, cap, wide):
    label, src, dst, far = INDEXED[k]
    case = far_case(arenas, 100 + k, src, dst, far)
    _core._copy_index_sync(*case.index_args(), 0, cap, wide_index=wide)
    case.check(f"{label} cap={cap} wide={wide}")


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("k", range(len(INDEXED)),
                         ids=[c[0] for c in INDEXED])
def test_indexed_far(arenas, k, cap):
    run_indexed(arenas, k, cap, False)


@pytest.mark.parametrize("k", range(len(INDEXED)),
                         ids=[c[0] for c in INDEXED])
def test_indexed_far_wide_index(arenas, k):
    run_indexed(arenas, k, 0, True)


def test_device_side_check_sees_a_byte_at_an_alias(arenas):
    """tests/test_guard_far_helper.py proves check() on host arenas; this
    is the same verdict where the arenas live. After a correct scatter,
    one byte put where a 32-bit offset would have sent it (past the base,
    and in the porch) fails check (b) by name."""
    label, src, dst, far = INDEXED[1]
    case = far_case(arenas, 199, src, dst, far)
    _core._copy_index_sync(*case.index_args(), 0)
    case.check(label)
    mod, minus, _ = aliases_of(case.di, dst.start, 2 ** 32)
    first_of_2050 = 2 * dst.slice_bytes
    assert dst.index[0] == 4100 and dst.index[2] == 2050
    for at, name in ((int(mod[0]), "offset modulo the modulus"),
                     (int(minus[first_of_2050]), "offset minus the modulus")):
        assert (at < 0) == (name == "offset minus the modulus")
        arenas.dst.region(at, 1).fill_(int(case.msg[0]))
        with pytest.raises(AssertionError,
                           match=f"arena offset {at}: .*{name}"):
            case.check(label)
        arenas.dst.region(at, 1).fill_(P)
    case.check(label)


# =============================================================================
# k_copy_nd (generic path) at far offsets
# =============================================================================

# (label, granule, far view, a far view of another shape for the other side)
ND_VIEWS = [
    ("16 B granule", 16,
     View(0, (3, 4, 24), (2 ** 31 + 512, 2 ** 24 + 96, 2), 2),
     View(0, (4, 3, 24), (1_440_000_000, 2 ** 20 + 96, 2), 2)),
    ("2 B granule", 2,
     View(0, (3, 4, 24), (2 ** 31 + 514, 2 ** 24 + 98, 2), 2),
     View(0, (4, 3, 24), (1_440_000_002, 2 ** 20 + 98, 2), 2)),
    ("1 B granule", 1,
     View(0, (3, 4, 25), (2 ** 31 + 513, 2 ** 24 + 97, 1), 1),
     View(0, (4, 3, 25), (1_440_000_001, 2 ** 20 + 97, 1), 1)),
    ("outer stride 2**32 + 4096 alone", 16,
     View(0, (2, 4, 24), (2 ** 32 + 4096, 64, 2), 2),
     View(0, (4, 2, 24), (1_440_000_000, 2 ** 20 + 96, 2), 2)),
]
DIRECTIONS = ["far -> near", "near -> far", "far -> far"]


def nd_sides(k, direction):
    _, g, v, other = ND_VIEWS[k]
    flat = View.dense(0, v.shape, v.itemsize)
    return {"far -> near": (v, flat, "s"), "near -> far": (flat, v, "d"),
            "far -> far": (v, other, "sd")}[direction]


def run_nd(arenas, k, direction, cap, wide):
    label, g = ND_VIEWS[k][:2]
    src, dst, far = nd_sides(k, direction)
    case = far_case(arenas, 200 + 3 * k + DIRECTIONS.index(direction), src,
                    dst, far)
    plans = [_core._plan_layout(list(v.shape), list(v.strides), v.itemsize, w)
             for v, w in ((src, False), (dst, True))]
    assert _core._plan_granule(*plans, case.src_ptr, case.dst_ptr) == g
    _core._copy_nd_sync(*case.nd_args(), 0, block_cap=cap, path="generic",
                        wide_index=wide)
    case.check(f"{label} {direction} cap={cap} wide={wide}")


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("k", range(len(ND_VIEWS)),
                         ids=[v[0] for v in ND_VIEWS])
def test_nd_generic_far(arenas, k, direction, cap):
    run_nd(arenas, k, direction, cap, False)


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("k", range(len(ND_VIEWS)),
                         ids=[v[0] for v in ND_VIEWS])
def test_nd_generic_far_wide_index(arenas, k, direction):
    run_nd(arenas, k, direction, 0, True)


# =============================================================================
# k_copy_nd_tile at far offsets
# =============================================================================

def tiled_views(E):
    return [
        # Rows 2 and 4 along B pass 2**31 and 2**32; 70 along A is ragged
        # over two (E = 2) or three (E = 16) tiles.
        ("far stride on B", View(0, (70, 5), (E, 2 ** 30 + 4096), E)),
        # 2**32 + 32768, not + 4096: batch 1 modulo 2**32 must not land on
        # a row of batch 0.
        ("far batch stride", View(0, (2, 70, 5), (2 ** 32 + 32768, E, 4096),
                                  E)),
    ]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("strided_is", ["source", "destination"])
@pytest.mark.parametrize("k", [0, 1], ids=["far stride on B",
                                           "far batch stride"])
@pytest.mark.parametrize("E", [2, 16])
def test_nd_tiled_far(arenas, E, k, strided_is, cap):
    label, v = tiled_views(E)[k]
    T = _core._ND_TILE[E][0]
    assert 70 % T and 70 > T, "A must be ragged over several tiles"
    flat = View.dense(0, v.shape, E)
    src, dst, far = (v, flat, "s") if strided_is == "source" \
        else (flat, v, "d")
    case = far_case(arenas, 300 + 8 * E + 2 * k + (far == "d"), src, dst, far)
    _core._copy_nd_sync(*case.nd_args(), 0, block_cap=cap, path="tiled")
    case.check(f"tiled E={E} {label}, strided {strided_is}, cap={cap}")


# =============================================================================
# k_copy_strided<16> and <1> at far offsets
# =============================================================================

def rows(row_bytes, stride) -> View:
    return View(0, (5, row_bytes), (stride, 1), 1)


# Five rows: rows 2 and 4 pass 2**31 and 2**32. The strides exceed 2**30 by
# more than a window, so that row 4 modulo 2**32 does not land on row 0.
STRIDED = [
    ("<16>", rows(1040, 2 ** 30 + 4096), rows(1040, 2 ** 30 + 8192)),
    ("<1>", rows(1041, 2 ** 30 + 4099), rows(1041, 2 ** 30 + 8197)),
]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("k", [0, 1], ids=[s[0] for s in STRIDED])
def test_strided_far(arenas, k, direction, cap):
    label, v, other = STRIDED[k]
    flat = View.dense(0, v.shape, 1)
    src, dst, far = {"far -> near": (v, flat, "s"),
                     "near -> far": (flat, v, "d"),
                     "far -> far": (v, other, "sd")}[direction]
    case = far_case(arenas, 400 + 3 * k + DIRECTIONS.index(direction), src,
                    dst, far)
    vec = all(s % 16 == 0 for s in (src.strides[0], dst.strides[0],
                                    v.shape[1]))
    assert vec == (label == "<16>")
    _core._copy_strided_sync(*case.strided_args(), 0, cap)
    case.check(f"k_copy_strided{label} {direction} cap={cap}")


# =============================================================================
# Whole messages past 4 GiB, generated and verified on the device
# =============================================================================

START = GUARD   # where the big regions begin, from the arena's base


def chunks(n, step=CHUNK):
    for c in range(0, n, step):
        yield slice(c, min(n, c + step))


def fill_random(region, seed):
    """Seeded random bytes, none equal to P."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for c in chunks(region.numel()):
        r = region[c]
        r.random_(0, 256, generator=gen)
        r.masked_fill_(r == P, P ^ 0xFF)


def prefill_unequal(region, want):
    """No byte of the destination equals the byte due to land on it."""
    for c in chunks(region.numel()):
        torch.bitwise_not(want[c], out=region[c])


def outside_is_constant(arenas, src_span, dst_span, label):
    for arena, span, what in ((arenas.dst, dst_span, "destination"),
                              (arenas.src, src_span, "source")):
        s = arena.stray(np.array([[START, START + span]]))
        assert s is None, (f"{label}: {s[0]} byte(s) of the {what} arena "
                           f"outside the message changed; first at arena "
                           f"offset {s[1]}: 0x{s[2]:02x}")


@pytest.mark.parametrize("count,wide", [(65, True), (63, False)],
                         ids=["n above 2**32: 64-bit index kernel",
                              "n just below 2**32: 32-bit kernel at its "
                              "largest"])
def test_indexed_real_size(arenas, count, wide):
    """`count` of 66 slices of 64 MiB + 1 bytes at a pitch of 64 MiB + 3,
    permuted, gathered into a dense run at granule 1."""
    S, pitch, slices = 64 * MIB + 1, 64 * MIB + 3, 66
    n = count * S
    assert (n > 2 ** 32 - 1) == wide and n > 2 ** 32 - 2 * S
    span = (slices - 1) * pitch + S
    assert START + span <= BODY
    arenas.src.fill()
    arenas.dst.fill()
    src = arenas.src.region(START, span)
    dst = arenas.dst.region(START, n)
    fill_random(src, 500 + count)
    idx = np.random.default_rng(count).permutation(slices)[:count]
    pool_view = src.as_strided((slices, S), (pitch, 1))
    want = pool_view[torch.from_numpy(idx).cuda()].reshape(-1)
    prefill_unequal(dst, want)
    torch.cuda.synchronize()
    _core._copy_index_sync(dst.data_ptr(), None, 0, 0, src.data_ptr(),
                           idx.tolist(), S, pitch, n, 0)
    assert torch.equal(dst, want), f"gather of {count} slices"
    del want
    outside_is_constant(arenas, span, n, f"gather of {count} slices")


@pytest.mark.parametrize("S,wide", [(64 * MIB + 1, True), (66_076_419, False)],
                         ids=["n above 2**32: 64-bit index kernel",
                              "n just below 2**32: 32-bit kernel at its "
                              "largest"])
def test_nd_real_size(arenas, S, wide):
    """A permuted byte view (13, 5, S) of a (5, 13, S) block, S odd, sent
    to contiguous at granule 1 through the production dispatch."""
    n = 65 * S
    assert S % 2 and (n > 2 ** 32 - 1) == wide and n > 2 ** 32 - 65
    assert START + n <= BODY
    arenas.src.fill()
    arenas.dst.fill()
    src = arenas.src.region(START, n)
    dst = arenas.dst.region(START, n)
    fill_random(src, 600 + wide)
    shape, strides = [13, 5, S], [S, 13 * S, 1]
    want = src.as_strided(shape, strides).contiguous().reshape(-1)
    prefill_unequal(dst, want)
    torch.cuda.synchronize()
    _core._copy_nd_sync(dst.data_ptr(), shape, [5 * S, S, 1], src.data_ptr(),
                        shape, strides, 1, 0)
    assert torch.equal(dst, want), f"permute, S={S}"
    del want
    outside_is_constant(arenas, n, n, f"permute, S={S}")


FLAT_N = 4 * GIB + 16 * 1000 + 5
# (label, source offset, destination offset, nbytes, tuning)
FLAT = [
    ("k_copy_b128<4,false>", 13, 13, FLAT_N,
     dict(nt_threshold=NEVER, stream_threshold=NEVER)),
    ("k_copy_b128<4,true>", 13, 13, FLAT_N,
     dict(nt_threshold=1, nt_unroll=4, stream_threshold=NEVER)),
    ("k_copy_b128<8,true>", 13, 13, FLAT_N,
     dict(nt_threshold=1, nt_unroll=8, stream_threshold=NEVER)),
    ("k_copy_stream", 13, 13, FLAT_N, dict(stream_threshold=1)),
    ("k_copy_elem<4>", 4, 8, FLAT_N - 1, {}),
    ("k_copy_elem<1>", 1, 2, FLAT_N, {}),
]


@pytest.mark.parametrize("k", range(len(FLAT)), ids=[f[0] for f in FLAT])
def test_flat_copy_past_4gib(arenas, k):
    label, soff, doff, n, tuning = FLAT[k]
    if soff % 16 == doff % 16:
        assert (16 - soff % 16) % 16 == 3, "a 3 B head"
    else:
        assert (soff % 4 == doff % 4 == 0 and n % 4 == 0) == ("<4>" in label)
    assert START + max(soff, doff) + n <= BODY
    arenas.src.fill()
    arenas.dst.fill()
    src = arenas.src.region(START + soff, n)
    dst = arenas.dst.region(START + doff, n)
    fill_random(src, 700)   # no byte equals P, which fills the destination
    torch.cuda.synchronize()
    _core._copy_device_sync(dst.data_ptr(), src.data_ptr(), n, 0, **tuning)
    assert torch.equal(dst, src), label
    for arena, off, what in ((arenas.dst, doff, "destination"),
                             (arenas.src, soff, "source")):
        s = arena.stray(np.array([[START + off, START + off + n]]))
        assert s is None, f"{label}: {what} arena changed outside: {s}"


ACCUM_N = 4 * GIB + 16 * 1000 + 4
# dtype -> (torch dtype, word dtype, exponent mask, top exponent bit, bits of 1)
ACCUM = {
    "int32": (torch.int32, torch.int32, 0, 0, 1),
    "bfloat16": (torch.bfloat16, torch.int16, 0x7F80, 0x4000, 0x3F80),
}


def reference_sum(d, s, td):
    if td == torch.int32:
        return d + s
    return (d.view(td).float() + s.view(td).float()).to(td).view(d.dtype)


@pytest.mark.parametrize("dtype", list(ACCUM))
def test_accumulate_past_4gib(arenas, dtype):
    """The input discipline of tests/_guard_accum.py, applied on the
    device: random bit patterns made finite, no sum equal to its
    destination. The reference is torch's sum, chunk by chunk; the
    comparison is on the raw words."""
    td, wd, exp, top, one = ACCUM[dtype]
    n = ACCUM_N
    arenas.src.fill()
    arenas.dst.fill()
    src = arenas.src.region(START, n)
    dst = arenas.dst.region(START, n)
    gen = torch.Generator(device="cuda").manual_seed(800 + len(dtype))
    want = torch.empty(n, dtype=torch.uint8, device="cuda").view(wd)
    sw, dw = src.view(wd), dst.view(wd)
    es = sw.element_size()
    for c in chunks(n // es, CHUNK // es):
        for region in (src, dst):
            region[c.start * es:c.stop * es].random_(0, 256, generator=gen)
        s, d = sw[c], dw[c]
        if exp:
            for w in (s, d):
                w.copy_(torch.where((w & exp) == exp, w & ~top, w))
        clash = reference_sum(d, s, td) == d
        s.masked_fill_(clash, one)
        d.masked_fill_(clash, one)
        ref = reference_sum(d, s, td)
        assert not (ref == d).any()
        if exp:
            assert not torch.isnan(ref.view(td).float()).any()
        want[c] = ref
    torch.cuda.synchronize()
    _core._accum_sync(dst.data_ptr(), src.data_ptr(), n, dtype, 0)
    assert torch.equal(dw, want), dtype
    del want
    outside_is_constant(arenas, n, n, f"accumulate {dtype}")
