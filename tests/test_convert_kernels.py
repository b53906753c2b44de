"""Bit-exact, guard-banded tests of the convert kernels (k_convert_vec,
k_convert_elem) and their dispatch (launch_convert), through the synchronous
hook ``_core._convert_sync``: all six ordered pairs of float32, float16 and
bfloat16, overwriting and accumulating, both lane shapes.

Sizes are derived from the kernels' shape, as in tests/test_accum_kernels.py:
256-thread workgroups, E elements per lane (8 for shape "a" and for
fp16 <-> bf16, 4 for shape "b"), a x4-unrolled grid-stride loop. With
``block_cap=2`` the grid stride is 512 lanes and one unrolled iteration
covers 2048, so the lane counts below sit on and around every boundary of
the grid, the unroll and the remainder loop, at tens of KiB per case. Each
case asks ``_core._convert_plan`` that head, lanes and tail are what it was
built for.

Expectation, inputs and the whole-arena verdict: tests/_guard_cast.py.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from starway_amd import _core  # noqa: E402

from _guard_cast import PAIRS, GuardedCast, itemsize  # noqa: E402

NVEC = [1, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 + 5]


def _variants():
    out = []
    for dst, src in PAIRS:
        shapes = ["a", "b"] if itemsize(dst) != itemsize(src) else [""]
        for shape in shapes:
            for acc in (False, True):
                out.append(pytest.param(
                    dst, src, shape, acc,
                    id=f"{src}-to-{dst}-{shape or 'x'}-"
                       f"{'accumulate' if acc else 'overwrite'}"))
    return out


VARIANTS = _variants()
variants = pytest.mark.parametrize("dst,src,shape,acc", VARIANTS)


def lane_elems(dst, src, shape):
    return 4 if shape == "b" and itemsize(dst) != itemsize(src) else 8


def offsets_for_head(dst, src, shape, head):
    """Byte offsets (source, destination) from a 256 B boundary at which
    the smallest co-aligning head is `head` elements."""
    E = lane_elems(dst, src, shape)
    ss, ds = itemsize(src), itemsize(dst)
    ps, pd = min(16, E * ss) // ss, min(16, E * ds) // ds
    assert head < max(ps, pd)
    return ((ps - head) % ps) * ss, ((pd - head) % pd) * ds


def run(case, shape, *, block_cap):
    _core._convert_sync(case.dst_ptr, case.src_ptr, case.n, case.dst_dtype,
                        case.src_dtype, 0, accumulate=case.accumulate,
                        block_cap=block_cap, shape=shape)


def plan(case, shape):
    return _core._convert_plan(case.dst_ptr, case.src_ptr, case.n,
                               case.dst_dtype, case.src_dtype, shape)


@variants
def test_head_bulk_tail_boundaries(dst, src, shape, acc):
    """Every lane count crossed with heads and tails of 0, 1 and E - 1."""
    E = lane_elems(dst, src, shape)
    seed = 500_000
    for nvec in NVEC:
        for head in (0, 1, E - 1):
            for tail in (0, 1, E - 1):
                seed += 1
                so, do = offsets_for_head(dst, src, shape, head)
                case = GuardedCast(seed, dst, src, head + E * nvec + tail,
                                   accumulate=acc, src_off=so, dst_off=do)
                assert plan(case, shape) == {
                    "kernel": "vector", "lane_elems": E, "head": head,
                    "vectors": nvec, "tail": tail}
                run(case, shape, block_cap=2)
                case.check(f"nvec={nvec} head={head} tail={tail}")


@variants
def test_single_block_many_iterations(dst, src, shape, acc):
    """block_cap=1: two unrolled iterations, three remainder ones and a
    ragged end, all by one workgroup."""
    E = lane_elems(dst, src, shape)
    nvec = 256 * 8 + 256 * 3 + 7
    so, do = offsets_for_head(dst, src, shape, E - 1)
    case = GuardedCast(510_000, dst, src, E - 1 + E * nvec + 1,
                       accumulate=acc, src_off=so, dst_off=do)
    assert plan(case, shape)["vectors"] == nvec
    run(case, shape, block_cap=1)
    case.check("block_cap=1")


@variants
def test_head_only(dst, src, shape, acc):
    """A message that ends before the first co-aligned boundary: the
    element kernel alone."""
    E = lane_elems(dst, src, shape)
    so, do = offsets_for_head(dst, src, shape, E - 1)
    for k, n in enumerate([1, E - 1]):
        case = GuardedCast(520_000 + k, dst, src, n, accumulate=acc,
                           src_off=so, dst_off=do)
        assert plan(case, shape) == {
            "kernel": "vector", "lane_elems": E, "head": n, "vectors": 0,
            "tail": 0}
        run(case, shape, block_cap=2)
        case.check(f"head only, n={n}")


@variants
def test_not_coalignable_takes_the_element_kernel(dst, src, shape, acc):
    ss, ds = itemsize(src), itemsize(dst)
    seed = 530_000
    for so, do in [(0, ds), (ss, 0)]:
        for n in [1, 255, 256, 257, 2 * 512 + 3]:
            seed += 1
            case = GuardedCast(seed, dst, src, n, accumulate=acc, src_off=so,
                               dst_off=do)
            assert plan(case, shape)["kernel"] == "element"
            run(case, shape, block_cap=2)
            case.check(f"src+{so} dst+{do} n={n}")


@variants
def test_zero_elements_is_a_noop(dst, src, shape, acc):
    case = GuardedCast(540_000, dst, src, 0, accumulate=acc,
                       src_off=itemsize(src))
    run(case, shape, block_cap=2)
    case.check_untouched("zero elements")


@pytest.mark.parametrize("dst,src", [("float32", "bfloat16"),
                                     ("bfloat16", "float32"),
                                     ("float16", "bfloat16")])
def test_default_tuning(dst, src):
    """The process-default grid and lane shape (what production launches),
    at about 64 KiB of message."""
    n = (64 << 10) // itemsize(src) + 13
    case = GuardedCast(550_000, dst, src, n, accumulate=True,
                       src_off=itemsize(src), dst_off=itemsize(dst))
    _core._convert_sync(case.dst_ptr, case.src_ptr, n, dst, src, 0,
                        accumulate=True)
    case.check("default tuning")


GIB = 1 << 30


@pytest.mark.parametrize("shape", ["a", "b"])
def test_wide_side_past_4gib(shape):
    """bf16 -> fp32 over 2**30 + 2051 elements: the destination's byte
    offsets pass 2**32 inside one launch. Generated and verified on the
    device with torch (widening is exact: the reference is .float()),
    bitwise, NaN patterns included; 256 guard bytes on either side of the
    destination keep their constant. Needs about 10 GiB; skipped when that
    does not fit."""
    n = GIB + 2051
    need = 10 * GIB
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need >> 30} GiB of free device memory, "
                    f"{free >> 30} GiB are free")
    guard = 64  # fp32 elements
    src = torch.empty(n, dtype=torch.int16, device="cuda")
    dst = torch.full((guard + n + guard,), 0x5A5A5A5A, dtype=torch.int32,
                     device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(560_000)
    step = 1 << 26
    for c in range(0, n, step):
        src[c:c + step].random_(-32768, 32768, generator=gen)
    torch.cuda.synchronize()
    body = dst[guard:guard + n]
    assert 4 * (n - 1) >= 2 ** 32
    assert _core._convert_plan(body.data_ptr(), src.data_ptr(), n, "float32",
                               "bfloat16", shape)["kernel"] == "vector"
    _core._convert_sync(body.data_ptr(), src.data_ptr(), n, "float32",
                        "bfloat16", 0, shape=shape)
    for c in range(0, n, step):
        want = src[c:c + step].view(torch.bfloat16).float().view(torch.int32)
        assert torch.equal(body[c:c + step], want), f"elements from {c}"
        del want
    assert (dst[:guard] == 0x5A5A5A5A).all()
    assert (dst[guard + n:] == 0x5A5A5A5A).all()
    del src, dst, body
    torch.cuda.empty_cache()
