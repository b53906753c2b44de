"""Direct, guard-banded, byte-exact tests of the three small-message
kernels in csrc/smallmsg.hip: k_inbox_push, k_inbox_unpack and the doorbell
k_inbox_wait, with every status word the doorbell can report.

The kernels are reached through the `_inbox_*` hooks, which call the host
functions the engine calls (inbox_create, same-process inbox_push,
inbox_unpack, arm_recv's two halves, arm_poll / arm_cancel / arm_free).

* Sources and destinations are tests/_guard.py arenas: seeded CPU bytes are
  the reference, the destination is prefilled so an unwritten byte cannot
  match, the WHOLE destination arena is compared with a numpy expectation
  and the source arena must be unchanged.
* The ring itself is checked the same way for the push kernel: it is seeded
  with a random pattern (complemented wherever it would equal the byte that
  is to land on it), and after the launch the whole ring must equal a
  host-built image -- header words, payload, and every untouched byte.
* Exact equality only. Ring geometry is read from the ring, never assumed.

Every spin in these kernels is iteration-bounded; no case here waits for
more than the kernels' own bounds (about 1 ms for the doorbell's default,
about 6 ms for the unpack kernel by the source's own estimate).
"""
import contextlib
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from starway_amd import _core  # noqa: E402

from _guard import GuardedCopy, Region  # noqa: E402

ALL = (1 << 64) - 1
T = 0x0123456789ABCDEF

COPIED, NOMATCH, CANCELED, EXPIRED = 1, 2, 3, 4


@contextlib.contextmanager
def inbox_ring():
    ring = _core._inbox_ring_create(0)
    try:
        yield ring
    finally:
        _core._inbox_ring_destroy(ring)


def _case(seed, nbytes, src_off=0, dst_off=0):
    return GuardedCopy(seed, Region.flat(src_off, nbytes),
                       Region.flat(dst_off, nbytes))


def _msg(case):
    """The message bytes of a case, from the host reference."""
    return case.src_host[case.src.start:case.src.start + case.src.nbytes]


def _assert_source_unchanged(case, label):
    now = case._fetch(case.src_buf)
    assert np.array_equal(now, case.src_host), f"{label}: source modified"


def _assert_untouched(case, label):
    """Nothing was delivered: the destination arena keeps its prefill."""
    got = case._fetch(case.dst_buf)
    bad = np.flatnonzero(got != case.dst_host)
    assert bad.size == 0, (
        f"{label}: {bad.size} destination byte(s) written, first at arena "
        f"offset {int(bad[0])} (message starts at {case.dst.start})")
    _assert_source_unchanged(case, label)


def _slot(ring, seq):
    return (seq % ring.slots) * ring.slot_bytes


def _push(ring, cases_seq_tag):
    _core._inbox_push_sync(
        ring, [(c.src_ptr, c.src.nbytes, seq, tag)
               for c, seq, tag in cases_seq_tag], 0)


# =============================================================================
# k_inbox_push: the whole ring against a host-built image
# =============================================================================


def _seed_ring(ring, seed, msgs):
    """Fill the ring with a seeded pattern that cannot pass for the result
    of pushing `msgs` [(case, seq, tag)]; return (seeded, expected)."""
    total = ring.slots * ring.slot_bytes
    image = np.random.default_rng(seed).integers(0, 256, total,
                                                 dtype=np.uint8)
    for case, seq, tag in msgs:
        size = case.src.nbytes
        o = _slot(ring, seq)
        hdr = np.frombuffer(struct.pack("<QQQ", seq, tag, size), np.uint8)
        clash = image[o:o + 24] == hdr
        image[o:o + 24][clash] ^= 0xFF
        p = o + ring.hdr_bytes
        clash = image[p:p + size] == _msg(case)
        image[p:p + size][clash] ^= 0xFF
    expected = image.copy()
    for case, seq, tag in msgs:
        size = case.src.nbytes
        o = _slot(ring, seq)
        expected[o:o + 24] = np.frombuffer(
            struct.pack("<QQQ", seq, tag, size), np.uint8)
        p = o + ring.hdr_bytes
        expected[p:p + size] = _msg(case)
    _core._inbox_ring_write(ring, 0, image)
    return image, expected


def _where_in_ring(ring, off):
    slot, rel = divmod(off, ring.slot_bytes)
    if rel < 24:
        part = ("seq", "tag", "size")[rel // 8] + " word"
    elif rel < ring.hdr_bytes:
        part = "header pad"
    else:
        part = f"payload byte {rel - ring.hdr_bytes}"
    return f"slot {slot} {part}"


def _check_ring(ring, expected, label):
    got = np.frombuffer(_core._inbox_ring_read(ring), np.uint8)
    assert got.size == expected.size
    bad = np.flatnonzero(got != expected)
    if bad.size:
        first = int(bad[0])
        raise AssertionError(
            f"{label}: {bad.size} wrong ring byte(s); first at "
            f"{_where_in_ring(ring, first)}: got 0x{int(got[first]):02x}, "
            f"expected 0x{int(expected[first]):02x}")


def _push_and_check(ring, seed, msgs, label):
    _, expected = _seed_ring(ring, seed, msgs)
    _push(ring, msgs)
    _check_ring(ring, expected, label)
    for case, _, _ in msgs:
        _assert_source_unchanged(case, label)


PUSH_SIZES = [0, 1, 15, 16, 17, 48, 255, 256, 4095, 4096]


@pytest.mark.parametrize("nbytes", PUSH_SIZES)
def test_push_single_message_layout(nbytes):
    """A. One message per launch: seq, tag and size words at 0, 8 and 16,
    header bytes 24..63 untouched, payload [0, size) from the source,
    payload [size, payload_max) untouched, every other slot untouched.
    The 16 B path needs a 16 B-aligned source and a size that is a
    multiple of 16: source offset 0 only. Offsets 1 and 8 take the byte
    path at every size."""
    with inbox_ring() as ring:
        assert nbytes <= ring.payload_max
        for k, src_off in enumerate([0, 1, 8]):
            case = _case(100 + nbytes * 4 + k, nbytes, src_off=src_off)
            seq = 7 + 3 * k
            _push_and_check(ring, 9000 + nbytes + k,
                            [(case, seq, T ^ (k << 60))],
                            f"push size={nbytes} src+{src_off}")


# 32 (size, source offset) pairs: both copy paths, empty and full payloads.
BATCH_SPECS = [
    (4096, 0), (0, 0), (1, 0), (15, 1), (16, 0), (16, 8), (17, 0), (48, 0),
    (48, 1), (255, 0), (256, 0), (256, 16), (256, 3), (1024, 0), (1000, 8),
    (4095, 0), (4095, 1), (4096, 1), (4096, 16), (64, 0), (64, 4), (2048, 0),
    (2047, 15), (3, 13), (0, 5), (32, 0), (33, 0), (512, 32), (511, 0),
    (4080, 0), (4080, 8), (128, 0),
]
assert len(BATCH_SPECS) == 32


def _batch(ring, n, base_seq, seed):
    """n messages in distinct slots, each with its own tag; bit 63 and bit
    32 of the tag are set on some."""
    out = []
    for i, (size, off) in enumerate(BATCH_SPECS[:n]):
        tag = (0xA000 + i) | ((i % 3 == 0) << 63) | ((i % 2 == 1) << 32)
        out.append((_case(seed + 17 * i, size, src_off=off),
                    base_seq + 2 * i, tag))
    assert len({_slot(ring, s) for _, s, _ in out}) == n
    return out


@pytest.mark.parametrize("n", [32, 1, 2, 31])
def test_push_batched_launch(n):
    """B. kPushMax descriptors in one launch, indexed by blockIdx.x: mixed
    sizes and source alignments, distinct slots, a distinct 64-bit tag per
    message. Also the batch sizes next to the edges."""
    with inbox_ring() as ring:
        msgs = _batch(ring, n, 3 * ring.slots + 1, 20_000 + n)
        assert any(t >> 63 for _, _, t in msgs)
        assert n == 1 or any((t >> 32) & 1 for _, _, t in msgs)
        _push_and_check(ring, 9100 + n, msgs, f"push batch n={n}")
        # Rotated, so other kinds sit in block 0 and in the last block.
        specs = msgs[::-1]
        specs = [(c, s + 5 * ring.slots, t ^ ALL) for c, s, t in specs]
        _push_and_check(ring, 9200 + n, specs, f"push batch n={n} reversed")


def test_push_sequence_numbers_around_the_ring():
    """C. Slot index 0 and slots-1, and 64-bit sequence numbers in the
    header word."""
    with inbox_ring() as ring:
        s = ring.slots
        seqs = [1, s - 1, s, s + 1, 2**32 + 5, 2**40 + s - 1]
        assert {q % s for q in seqs} >= {0, s - 1}
        for k, seq in enumerate(seqs):
            case = _case(300 + k, 100 + k, src_off=k % 2)
            _push_and_check(ring, 9300 + k, [(case, seq, T + k)],
                            f"push seq={seq}")
        # One launch for the four of them that land in distinct slots
        # (0, 1, 5 and s-1).
        batch = [(_case(310 + k, 64 + k), seq, T - k)
                 for k, seq in enumerate(seqs) if seq not in (1, s - 1)]
        assert len({_slot(ring, q) for _, q, _ in batch}) == len(batch) == 4
        _push_and_check(ring, 9310, batch, "push seqs batched")


# =============================================================================
# k_inbox_unpack: a full batch with four payloads that never arrive
# =============================================================================


def test_unpack_batched_with_missing_neighbours():
    """D. 32 descriptors in one launch after a matching push: 28 delivered
    (16 B-aligned and odd destinations and sizes, size 0, three pinned
    bounces) next to four that never arrive -- two empty slots, one slot
    holding the previous epoch and one holding the next. The four report
    status 2 with untouched destinations; the 28 report 1 with exact
    bytes. The only case that waits out the unpack kernel's spin bound."""
    with inbox_ring() as ring:
        s = ring.slots
        base = 2 * s + 1
        empty = {4, 19}
        prev_epoch, next_epoch = 9, 30
        bounce = {2, 13, 31}
        dst_offs = [0, 1, 3, 8, 16, 5]
        cases, seqs = [], []
        for i, (size, off) in enumerate(BATCH_SPECS):
            cases.append(_case(30_000 + 13 * i, size, src_off=off,
                               dst_off=dst_offs[i % len(dst_offs)]))
            seqs.append(base + i)
        assert all(cases[i].src.nbytes > 0
                   for i in empty | {prev_epoch, next_epoch})
        assert any(c.src.nbytes == 0 for c in cases)
        push = []
        for i, (c, q) in enumerate(zip(cases, seqs)):
            if i in empty:
                continue
            if i == prev_epoch:
                q -= s
            elif i == next_epoch:
                q += s
            push.append((c, q, 0xB000 + i))
        assert len(push) == 30
        _push(ring, push)
        res = _core._inbox_unpack_sync(
            ring, [(q, c.src.nbytes, 0 if i in bounce else c.dst_ptr)
                   for i, (c, q) in enumerate(zip(cases, seqs))])
        assert len(res) == 32
        missing = empty | {prev_epoch, next_epoch}
        for i, ((status, staged), c) in enumerate(zip(res, cases)):
            label = f"unpack desc {i} size={c.src.nbytes} dst+{c.dst.off}"
            if i in missing:
                assert status == 2, label
                _assert_untouched(c, label)
            elif i in bounce:
                assert status == 1, label
                assert staged == _msg(c).tobytes(), label
                _assert_untouched(c, label)
            else:
                assert status == 1, label
                assert staged is None
                c.check(label)
        # Two kinds the batch above does not hold: one 16 B element through
        # the vector branch, and a full payload whose destination is one
        # byte off 16 B alignment.
        edge = [_case(31_000, 16), _case(31_001, ring.payload_max, dst_off=1)]
        seqs = [base + 2 * s, base + 2 * s + 1]
        _push(ring, [(c, q, 0xC000 + i)
                     for i, (c, q) in enumerate(zip(edge, seqs))])
        res = _core._inbox_unpack_sync(
            ring, [(q, c.src.nbytes, c.dst_ptr) for c, q in zip(edge, seqs)])
        assert res == [(1, None), (1, None)]
        for c in edge:
            c.check(f"unpack edge size={c.src.nbytes} dst+{c.dst.off}")


# =============================================================================
# k_inbox_wait: every status word
# =============================================================================


def _arm(ring, seq, tag, mask, case, max_size=None, **kw):
    if max_size is None:
        max_size = case.dst.nbytes
    return _core._inbox_arm_begin(ring, seq, tag, mask, case.dst_ptr,
                                  max_size, **kw)


def _unpack_delivers(ring, seq, case, label):
    """The slot is intact: the ordinary path still delivers it exactly."""
    res = _core._inbox_unpack_sync(ring,
                                   [(seq, case.src.nbytes, case.dst_ptr)])
    assert res == [(1, None)], label
    case.check(label)


WAIT_SIZES = [0, 1, 15, 16, 17, 255, 256, 4095, 4096]


@pytest.mark.parametrize("nbytes", WAIT_SIZES)
def test_wait_prepublished_match(nbytes):
    """E. The message is in the slot before the doorbell starts. Offsets
    1 and 3 and the odd sizes take the byte path. With a buffer larger
    than the message only `size` bytes change (the extra 37 bytes of
    capacity lie inside the arena's trailing guard)."""
    with inbox_ring() as ring:
        seq = ring.slots + 3
        for dst_off in [0, 1, 3, 8]:
            for extra in [0, 37]:
                seq += 1
                case = _case(40_000 + nbytes * 8 + dst_off + extra, nbytes,
                             src_off=dst_off % 2, dst_off=dst_off)
                _push(ring, [(case, seq, T)])
                t = _arm(ring, seq, T, ALL, case, max_size=nbytes + extra)
                assert _core._inbox_arm_end(t) == (COPIED, nbytes)
                case.check(f"wait size={nbytes} dst+{dst_off} "
                           f"max={nbytes + extra}")


MATCH_ROWS = [
    # recv tag, mask, message tag, expected status
    pytest.param(T, ALL, T, COPIED, id="exact"),
    pytest.param(T, ALL, T ^ (1 << 63), NOMATCH, id="bit63_differs"),
    pytest.param(T, ALL, T ^ (1 << 32), NOMATCH, id="bit32_differs"),
    pytest.param(T, (1 << 32) - 1, T ^ (1 << 40), COPIED, id="low32_mask"),
    pytest.param(0xDEAD, 0, ALL ^ 0x55, COPIED, id="wildcard"),
]


@pytest.mark.parametrize("rtag,mask,mtag,want", MATCH_ROWS)
def test_wait_match_logic(rtag, mask, mtag, want):
    """F. 64-bit tag and mask compares at 64 B. A nomatch leaves the
    destination untouched and the slot intact: the unpack kernel still
    delivers the message exactly (the engine's nomatch contract)."""
    with inbox_ring() as ring:
        seq = 2**33 + 11
        case = _case(50_000 + want + (mask & 0xFF), 64)
        _push(ring, [(case, seq, mtag)])
        t = _arm(ring, seq, rtag, mask, case)
        if want == COPIED:
            assert _core._inbox_arm_end(t) == (COPIED, 64)
            case.check("wait match")
        else:
            assert _core._inbox_arm_end(t) == (NOMATCH, 0)
            _assert_untouched(case, "wait nomatch")
            _unpack_delivers(ring, seq, case, "unpack after nomatch")


def test_wait_oversize_is_nomatch():
    """F. A message one byte longer than the armed buffer is left alone."""
    with inbox_ring() as ring:
        seq = 70
        case = _case(50_100, 65)
        _push(ring, [(case, seq, T)])
        t = _arm(ring, seq, T, ALL, case, max_size=64)
        assert _core._inbox_arm_end(t) == (NOMATCH, 0)
        _assert_untouched(case, "wait oversize")
        _unpack_delivers(ring, seq, case, "unpack after oversize")


def test_wait_canceled_before_start_never_copies():
    """G. The cancel word is set before the launch is enqueued and the
    matching message is already published. A doorbell that starts canceled
    belongs to a recv the engine has handed to another delivery path: it
    must report 3, leave the destination alone and leave the slot to the
    ordinary path.

    k_inbox_wait without the cancel read on entry tests the slot first and
    polls the cancel word only every 64th iteration, so it reports 1 and
    copies here."""
    with inbox_ring() as ring:
        seq = 2 * ring.slots + 9
        case = _case(60_000, 200, dst_off=3)
        _push(ring, [(case, seq, T)])
        t = _arm(ring, seq, T, ALL, case, precancel=True)
        status = _core._inbox_arm_end(t)
        _assert_untouched(case, f"wait precanceled (status {status})")
        assert status == (CANCELED, 0)
        _unpack_delivers(ring, seq, case, "unpack after precancel")


def test_wait_canceled_while_spinning():
    """H. Empty slot and a bound of 400 000 iterations (about 50 ms by the
    source's "8000 is about 1 ms", which nobody has measured): a cancel
    right after the launch must end the kernel with 3, not let it run to
    4. Whether the kernel had started when the cancel landed does not
    matter: both the entry check and the in-loop poll report 3."""
    with inbox_ring() as ring:
        case = _case(60_100, 64)
        t = _arm(ring, 5, T, ALL, case, spin_iters=400_000)
        _core._inbox_arm_cancel(t)
        assert _core._inbox_arm_end(t) == (CANCELED, 0)
        _assert_untouched(case, "wait canceled")


@pytest.mark.parametrize("slot_state", ["empty", "previous_epoch",
                                        "next_epoch", "other_high_word"])
def test_wait_expires(slot_state):
    """I. Default bound. A slot that is empty, or that holds the message
    of another ring epoch (same slot index, other sequence number, same
    tag), never matches: status 4, destination untouched. The last state
    differs from the expected sequence number in bit 32 only."""
    with inbox_ring() as ring:
        seq = 3 * ring.slots + 17
        case = _case(60_200 + len(slot_state), 96, dst_off=1)
        if slot_state != "empty":
            other = {"previous_epoch": seq - ring.slots,
                     "next_epoch": seq + ring.slots,
                     "other_high_word": seq + 2**32}[slot_state]
            assert _slot(ring, other) == _slot(ring, seq)
            _push(ring, [(case, other, T)])
        t = _arm(ring, seq, T, ALL, case)
        assert _core._inbox_arm_end(t) == (EXPIRED, 0)
        _assert_untouched(case, f"wait expiry, slot {slot_state}")


def test_wait_armed_then_pushed():
    """J. The doorbell is resident (or queued) when the message is pushed.
    The push and wait streams may share a hardware queue, in which case
    the push is held until the wait expires; so two outcomes are legal and
    each is checked in full:
      * 1 with exact bytes;
      * 4 with the destination untouched, after which a second doorbell
        on the now-published slot reports 1 with exact bytes."""
    with inbox_ring() as ring:
        seq = ring.slots + 2
        case = _case(60_300, 777, src_off=1, dst_off=8)
        t = _arm(ring, seq, T, ALL, case)
        _push(ring, [(case, seq, T)])
        status = _core._inbox_arm_end(t)
        print(f"armed-then-pushed: first doorbell reported {status}")
        if status == (EXPIRED, 0):
            _assert_untouched(case, "wait expired before the push ran")
            t = _arm(ring, seq, T, ALL, case)
            status = _core._inbox_arm_end(t)
        assert status == (COPIED, 777)
        case.check("wait armed then pushed")
