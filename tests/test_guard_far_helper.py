"""tests/_guard_far.py itself, on host arenas with a wrap modulus of 2**16
(a 32 KiB porch and a 68 KiB body): the window merging, the alias
assertion, the numpy expectation, and the proof that check() passes for a
correct copy and fails, with the right text, for each of the three
wrong-address models the far GPU tests are for.
"""
import numpy as np
import pytest

from _guard_far import (ALIASES, GUARD, P, FarArenas, GuardedFar, Pool, View,
                        aliases_of, dense, geometry, windows_of)

M = 2 ** 16

# Slices of 48 B at a pitch of 1040 B: entry 33 passes M / 2, entries 64
# and 65 pass M; the scaled-down picture of the GPU tests' large-pitch pool.
POOL = Pool(0, 66, 48, 1040, (65, 0, 33, 64, 3, 34))
# A (3, 4, 24) byte view whose outer stride is M / 2 + 1024; its rows of 24
# sit 96 B apart, so each outer index makes one window.
ND = View(0, (3, 4, 24), (M // 2 + 1024, 96, 1), 1)


@pytest.fixture(scope="module")
def arenas():
    return FarArenas(M, src_on_host=True, dst_on_host=True)


def _copy(case, src_at=None, dst_at=None):
    """The copy under test, done by hand: byte by byte in message order,
    reading at `src_at` and writing at `dst_at` (default: the right
    offsets)."""
    a = case.arenas
    src_at = case.si if src_at is None else src_at
    dst_at = case.di if dst_at is None else dst_at
    a.dst.buf[a.dst.porch + dst_at] = a.src.buf[a.src.porch + src_at]


def test_geometry_and_constants():
    assert geometry(2 ** 32) == (2 << 30, (4 << 30) + (256 << 20))
    assert geometry(M) == (32768, 69632)
    assert (P, GUARD) == (0xA5, 256)


def test_windows_widen_and_merge_where_they_meet():
    run = np.arange(1000, 1010)
    assert windows_of(run).tolist() == [[1000 - GUARD, 1010 + GUARD]]
    # A gap of exactly 2 * GUARD bytes: the widened runs touch and merge.
    meet = np.concatenate((run, run + 10 + 2 * GUARD))
    assert windows_of(meet).tolist() == \
        [[1000 - GUARD, 1020 + 3 * GUARD]]
    # One byte more: two windows with one constant byte between them.
    apart = np.concatenate((run, run + 11 + 2 * GUARD))
    assert windows_of(apart).tolist() == \
        [[1000 - GUARD, 1010 + GUARD], [1011 + GUARD, 1021 + 3 * GUARD]]
    # Message order and repeats do not matter.
    assert windows_of(meet[::-1].repeat(2)).tolist() == \
        windows_of(meet).tolist()
    assert windows_of(np.empty(0, dtype=np.int64)).shape == (0, 2)
    assert len(windows_of(POOL.indices())) == 6
    assert len(windows_of(ND.indices())) == 3


def test_aliases_are_taken_from_the_kernel_pointer():
    start = 300
    offs = start + np.array([5, M // 2 + 5, M + 5])
    mod, minus, sext = aliases_of(offs, start, M)
    assert mod.tolist() == [305, start + M // 2 + 5, 305]
    assert minus.tolist() == [305 - M, start - M // 2 + 5, 305]
    assert sext.tolist() == [305, start - M // 2 + 5, 305]


def test_alias_in_a_window_rejects_the_case(arenas):
    # Entry 64 at a pitch of 1024 lies exactly one modulus above entry 0.
    bad = Pool(0, 66, 48, 1024, (64, 0, 33))
    with pytest.raises(AssertionError,
                       match=r"alias \(offset modulo the modulus\) of "
                             r"offset \d+ at \d+ falls in a window"):
        GuardedFar(arenas, 1, bad, dense(0, bad.nbytes))
    with pytest.raises(AssertionError, match="falls in a window"):
        GuardedFar(arenas, 1, dense(0, bad.nbytes), bad)
    # Entry 67 ends past the body.
    with pytest.raises(AssertionError, match="does not fit the arena"):
        GuardedFar(arenas, 1, Pool(0, 68, 48, 1040, (67, 0)), dense(0, 96))
    GuardedFar(arenas, 1, POOL, dense(0, POOL.nbytes))   # this one is fine


def test_expectation_and_inputs(arenas):
    case = GuardedFar(arenas, 2, POOL, ND.permute((1, 0, 2)))
    assert case.crosses(POOL) and case.crosses(case.dst)
    assert not case.crosses(dense(0, 64))
    a = arenas
    # Nothing in the source message equals P; no destination byte already
    # holds what is to land on it; everything outside the windows is P.
    msg = a.src.buf[a.src.porch + case.si]
    assert np.array_equal(msg, case.msg) and not (msg == P).any()
    assert not (a.dst.buf[a.dst.porch + case.di] == msg).any()
    inside = np.zeros(a.dst.buf.size, dtype=bool)
    for lo, hi in case.dpack.windows:
        inside[a.dst.porch + lo:a.dst.porch + hi] = True
    assert (a.dst.buf[~inside] == P).all()
    assert a.dst.stray(case.dpack.windows) is None
    case.check_untouched()
    with pytest.raises(AssertionError, match="wrong destination byte"):
        case.check("nothing copied")
    want = a.dst.buf.copy()
    want[a.dst.porch + case.di] = msg
    _copy(case)
    assert np.array_equal(a.dst.buf, want)
    case.check("copied")
    with pytest.raises(AssertionError, match="was written"):
        case.check_untouched()


CASES = [
    ("gather", POOL, dense(0, POOL.nbytes)),
    ("scatter", dense(0, POOL.nbytes), POOL),
    ("N-D window", dense(0, ND.nbytes), ND),
    ("both far", POOL, Pool(16, 66, 96, 1040, (64, 2, 34))),
]


@pytest.mark.parametrize("label,src,dst", CASES, ids=[c[0] for c in CASES])
def test_correct_copy_passes(arenas, label, src, dst):
    case = GuardedFar(arenas, 3, src, dst)
    _copy(case)
    case.check(label)


@pytest.mark.parametrize("model", range(3), ids=ALIASES)
@pytest.mark.parametrize("label,src,dst", CASES[1:],
                         ids=[c[0] for c in CASES[1:]])
def test_wrong_destination_address_fails(arenas, label, src, dst, model):
    """The three broken kernels: every destination offset formed modulo the
    modulus, minus the modulus (from M / 2 on, where a signed narrow
    product goes wrong), or from its sign-extended low half."""
    case = GuardedFar(arenas, 4, src, dst)
    al = aliases_of(case.di, dst.start, M)[model].copy()
    if model == 1:
        near = case.di - dst.start < M // 2
        al[near] = case.di[near]
    assert (al != case.di).any()
    _copy(case, dst_at=al)
    with pytest.raises(AssertionError) as e:
        case.check(label)
    text = str(e.value)
    assert "wrong destination byte" in text           # (a): never arrived
    assert "destination arena outside its windows changed" in text   # (b)
    assert ALIASES[model] in text and "of message byte" in text
    assert "source" not in text.split(" [src ")[0]


@pytest.mark.parametrize("model", range(3), ids=ALIASES)
def test_wrong_source_address_fails(arenas, model):
    """A broken read fetches the constant, which no message byte equals."""
    case = GuardedFar(arenas, 5, POOL, dense(0, POOL.nbytes))
    al = aliases_of(case.si, POOL.start, M)[model].copy()
    if model == 1:
        near = case.si - POOL.start < M // 2
        al[near] = case.si[near]
    _copy(case, src_at=al)
    with pytest.raises(AssertionError,
                       match="wrong destination byte.*got 0xa5"):
        case.check()


def test_stray_and_source_writes_are_named(arenas):
    case = GuardedFar(arenas, 6, POOL, dense(0, POOL.nbytes))
    _copy(case)
    case.check()
    a = arenas
    a.dst.buf[a.dst.porch + 40000] ^= 1
    with pytest.raises(AssertionError,
                       match="1 byte.s. of the destination arena outside "
                             "its windows changed; first at arena offset "
                             "40000: 0xa4, no alias"):
        case.check()
    a.dst.buf[a.dst.porch + 40000] ^= 1
    a.dst.buf[0] ^= 1                       # the first byte of the porch
    with pytest.raises(AssertionError, match=f"arena offset {-M // 2}"):
        case.check()
    a.dst.buf[0] ^= 1
    a.dst.buf[a.dst.porch + GUARD - 1] ^= 1     # guard in front of the run
    with pytest.raises(AssertionError, match="guard or gap"):
        case.check()
    a.dst.buf[a.dst.porch + GUARD - 1] ^= 1
    a.src.buf[-1] ^= 1                       # the last byte of the body
    with pytest.raises(AssertionError, match="source arena outside"):
        case.check()
    a.src.buf[-1] ^= 1
    a.src.buf[a.src.porch + int(case.si[7])] ^= 1
    with pytest.raises(AssertionError, match="wrong source byte"):
        case.check()
    a.src.buf[a.src.porch + int(case.si[7])] ^= 1
    case.check("restored")
