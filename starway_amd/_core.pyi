"""Typed surface of the native module (parity contract with the reference's
src/starway/_bindings.pyi, extended: buffers may be host arrays (buffer
protocol) OR device tensors (__cuda_array_interface__)."""
from collections.abc import Callable
from typing import Any

Buffer = Any  # numpy ndarray / buffer protocol object / __cuda_array_interface__

class Context:
    def __init__(self) -> None: ...

class ServerEndpoint:
    @property
    def name(self) -> str: ...
    @property
    def local_addr(self) -> str: ...
    @property
    def local_port(self) -> int: ...
    @property
    def remote_addr(self) -> str: ...
    @property
    def remote_port(self) -> int: ...
    def view_transports(self) -> list[tuple[str, str]]: ...

class Server:
    def __init__(self, ctx: Context) -> None: ...
    def set_accept_callback(
        self, callback: Callable[[ServerEndpoint], None]
    ) -> None: ...
    def listen(self, addr: str, port: int) -> None: ...
    def listen_address(self) -> None: ...
    def get_worker_address(self) -> bytes: ...
    def close(self, callback: Callable[[], None]) -> None: ...
    def send(
        self,
        client_ep: ServerEndpoint,
        buffer: Buffer,
        tag: int,
        done_callback: Callable[[], None],
        fail_callback: Callable[[str], None],
        index: Index | None = None,
    ) -> None:
        """index=idx: the message is the slices buffer[idx[0]],
        buffer[idx[1]], ... of a device tensor (see recv)."""
    def recv(
        self,
        buffer: Buffer,
        tag: int,
        tag_mask: int,
        done_callback: Callable[[int, int], None],
        fail_callback: Callable[[str], None],
        reduce: str = "",
        dtype: str = "",
        index: Index | None = None,
        msg_dtype: str = "",
    ) -> None:
        """reduce="sum" with dtype float32 / float16 / bfloat16 / int32: a
        reducing receive, buf[i] += msg[i] over length // itemsize elements.
        ValueError for an unknown op, a host buffer, another dtype, a
        non-contiguous destination or one not aligned to its item size.

        msg_dtype (float32 / float16 / bfloat16) with dtype, the buffer's
        own, another of the three: a converting receive. The message is
        read as msg_dtype elements and converted in the kernel, buf[i] =
        dtype(msg[i]), or with reduce="sum" dtype(float(buf[i]) +
        float(msg[i])), over length // msg_itemsize elements. Equal names
        are the receive without msg_dtype. ValueError starting "msg_dtype
        limit:" for another name (checked before the buffer is looked at),
        a host buffer, another buffer dtype, a non-contiguous or
        item-misaligned destination, or index= with msg_dtype=.

        index=idx: message slice r is written to buffer[idx[r]]. The buffer
        is a device tensor exporting its own shape and byte strides, dense
        after the first dimension; idx is a host-side sequence of ints, 1-D
        numpy integer array or 1-D CPU torch integer tensor, validated and
        copied here. ValueError starting "index limit:" for a host buffer,
        a device / bool / float / non-1-D index, an entry out of range, a
        repeated destination entry, more than _INDEX_MAX entries, non-dense
        slices, overlapping destination slices, or index= with reduce=."""
    def flush(
        self, done_callback: Callable[[], None], fail_callback: Callable[[str], None]
    ) -> None: ...
    def flush_ep(
        self,
        client_ep: ServerEndpoint,
        done_callback: Callable[[], None],
        fail_callback: Callable[[str], None],
    ) -> None: ...
    def list_clients(self) -> set[ServerEndpoint]: ...
    def get_stats(self) -> dict[str, int]: ...
    def evaluate_perf(self, client_ep: ServerEndpoint, msg_size: int) -> float: ...

class Client:
    def __init__(self, ctx: Context) -> None: ...
    def connect(
        self, addr: str, port: int, callback: Callable[[str], None]
    ) -> None: ...
    def connect_address(
        self, remote_address: bytes, callback: Callable[[str], None]
    ) -> None: ...
    def get_worker_address(self) -> bytes: ...
    def close(self, callback: Callable[[], None]) -> None: ...
    def send(
        self,
        buffer: Buffer,
        tag: int,
        done_callback: Callable[[], None],
        fail_callback: Callable[[str], None],
        index: Index | None = None,
    ) -> None:
        """index=idx: the message is the slices buffer[idx[0]],
        buffer[idx[1]], ... of a device tensor (see recv)."""
    def recv(
        self,
        buffer: Buffer,
        tag: int,
        tag_mask: int,
        done_callback: Callable[[int, int], None],
        fail_callback: Callable[[str], None],
        reduce: str = "",
        dtype: str = "",
        index: Index | None = None,
        msg_dtype: str = "",
    ) -> None:
        """reduce="sum" with dtype float32 / float16 / bfloat16 / int32: a
        reducing receive, buf[i] += msg[i] over length // itemsize elements.
        ValueError for an unknown op, a host buffer, another dtype, a
        non-contiguous destination or one not aligned to its item size.

        msg_dtype (float32 / float16 / bfloat16) with dtype, the buffer's
        own, another of the three: a converting receive. The message is
        read as msg_dtype elements and converted in the kernel, buf[i] =
        dtype(msg[i]), or with reduce="sum" dtype(float(buf[i]) +
        float(msg[i])), over length // msg_itemsize elements. Equal names
        are the receive without msg_dtype. ValueError starting "msg_dtype
        limit:" for another name (checked before the buffer is looked at),
        a host buffer, another buffer dtype, a non-contiguous or
        item-misaligned destination, or index= with msg_dtype=.

        index=idx: message slice r is written to buffer[idx[r]]. The buffer
        is a device tensor exporting its own shape and byte strides, dense
        after the first dimension; idx is a host-side sequence of ints, 1-D
        numpy integer array or 1-D CPU torch integer tensor, validated and
        copied here. ValueError starting "index limit:" for a host buffer,
        a device / bool / float / non-1-D index, an entry out of range, a
        repeated destination entry, more than _INDEX_MAX entries, non-dense
        slices, overlapping destination slices, or index= with reduce=."""
    def flush(
        self, done_callback: Callable[[], None], fail_callback: Callable[[str], None]
    ) -> None: ...
    def get_stats(self) -> dict[str, int]: ...
    def evaluate_perf(self, msg_size: int) -> float: ...

def gpu_available() -> bool: ...
def ipc_invalidate() -> None: ...
def calibrate(force: bool = False) -> dict[str, float]: ...
def gpu_device_count() -> int: ...
def _copy_device_sync(
    dst: int, src: int, nbytes: int, device: int, block_cap: int = 0,
    nt_threshold: int = 0, nt_unroll: int = 0,
) -> None: ...
def _copy_strided_sync(
    dst: int, dst_stride: int, src: int, src_stride: int, rows: int,
    row_bytes: int, device: int, block_cap: int = 0,
) -> None: ...
def _copy_multi_sync(
    descs: list[tuple[int, int, int]], device: int
) -> None: ...
def _accum_sync(
    dst: int, src: int, nbytes: int, dtype: str, device: int,
    block_cap: int = 0, nt_threshold: int = 0,
) -> None:
    """Run the accumulate kernels (k_accum_b128 / k_accum_elem)
    synchronously on raw device pointers: dst[i] += src[i] over nbytes //
    itemsize elements of dtype (float32, float16, bfloat16, int32).
    nt_threshold is the accumulate family's own (bulk bytes from which the
    source loads are non-temporal; 0 = the process default, 192 MiB).
    ValueError for another dtype, or pointers / a length that are not
    multiples of the item size."""

def _convert_sync(
    dst: int, src: int, n_elems: int, dst_dtype: str, src_dtype: str,
    device: int, *, accumulate: bool = False, block_cap: int = 0,
    shape: str = "", nt_threshold: int = 0,
) -> None:
    """Run the convert kernels (k_convert_vec / k_convert_elem)
    synchronously on raw device pointers: dst[i] = dst_dtype(src[i]), or
    with accumulate dst_dtype(float(dst[i]) + float(src[i])), over n_elems
    elements. The dtypes are two different ones of float32, float16,
    bfloat16. shape picks the lane shape of a 2-byte <-> 4-byte pair: "a"
    (8 elements per lane), "b" (4) or "" (what production runs). The family
    has no non-temporal variant: nt_threshold takes 0 only. ValueError,
    before any device is touched, for anything else, equal dtypes or a
    pointer that is not a multiple of its item size."""

def _convert_plan(
    dst: int, src: int, n_elems: int, dst_dtype: str, src_dtype: str,
    shape: str = "",
) -> dict[str, Any]:
    """How the convert dispatch splits such a message: kernel ("vector" or
    "element"), lane_elems, head, vectors, tail. "element" means no head
    co-aligns the two sides and the element kernel takes all n_elems
    (reported as tail). Host only."""

def _convert_shape(shape: str | None = None) -> str:
    """The lane shape ("a" or "b") that shape="" resolves to: the
    production shape, unless a bench has set another with this call (""
    restores it). Host only."""

def _copy_tuning() -> dict[str, int]: ...
def _copy_stream_tuning() -> dict[str, int]:
    """Streaming-kernel defaults (csrc/copy_stream.hpp): stream_threshold,
    stream_blocks and unroll, the production kernel's elements per lane per
    tile (a tile is 256 * unroll elements of 16 B). Host only."""

def _copy_stream_plan(
    n16: int, stream_blocks: int = 0, block: int | None = None
) -> dict[str, int]:
    """Tile plan of the production streaming kernel for n16 bulk elements
    under a grid cap (0 = the process default): tile, full_tiles, ragged,
    tiles, grid. With `block`, also that workgroup's first_tile, last_tile
    and n_tiles (it takes every grid-th tile from first_tile). ValueError
    when the cap resolves to 0. Host only."""

# N-D layouts (csrc/layout.hpp). A plan is (unit, [(extent, stride_bytes),
# ...]): `unit` bytes of dense innermost run, then the dimensions outside
# it, outermost first; an empty list means contiguous. Message byte m lives
# at offset (m % unit) + sum(idx_d * stride_d), idx peeled from m // unit
# innermost first.
_Plan = tuple[int, list[tuple[int, int]]]

def _plan_layout(
    shape: list[int], strides_bytes: list[int], itemsize: int,
    writable: bool = False,
) -> _Plan:
    """Normalise a view: drop size-1 dimensions, merge neighbours, fold a
    dense innermost dimension into `unit`. ValueError for negative strides,
    more than _ND_MAX_DIMS remaining dimensions and, with writable=True,
    overlapping elements. Host only: works without a GPU."""

def _plan_granule(
    src_plan: _Plan, dst_plan: _Plan, src_ptr: int, dst_ptr: int
) -> int:
    """Largest power of two <= 16 dividing both units, every stride and
    both addresses: the access width k_copy_nd runs with. Host only."""

def _copy_nd_sync(
    dst: int, dst_shape: list[int], dst_strides: list[int],
    src: int, src_shape: list[int], src_strides: list[int],
    itemsize: int, device: int, block_cap: int = 0, path: str = "auto",
    wide_index: bool = False,
) -> None:
    """Run the N-D copy kernels synchronously on raw device pointers
    (strides in bytes). path: "auto" (the production dispatch), "generic"
    (k_copy_nd) or "tiled" (k_copy_nd_tile; ValueError when the pair is not
    in the transpose family). wide_index runs k_copy_nd's 64-bit index
    instantiation, which production takes only past 2**32 - 1 granules."""

# k_copy_nd_tile tile extents: element bytes -> (T_A, T_B) in elements.
_ND_TILE: dict[int, tuple[int, int]]
_ND_MAX_DIMS: int

# Indexed buffers (csrc/index.hpp). All but _copy_index_sync are host-only.
Index = Any  # sequence of ints, 1-D numpy integer array, 1-D CPU torch tensor
_INDEX_MAX: int  # kIndexMax: most entries one index list may hold
_RTS_DESC_BYTES: int  # sizeof(RtsDesc)
_PROTO_VERSION: int
_FT_RTS_INDEXED: int

def _plan_index(index: Index, extent: int, writable: bool = False) -> list[int]:
    """The validated u32 list for a buffer of `extent` slices, or ValueError
    ("index limit: ..."); writable=True also refuses a repeated entry."""

def _index_offset(index: list[int], slice_bytes: int, stride: int, m: int) -> int:
    """Byte offset from the buffer's base of message byte m:
    index[m // slice_bytes] * stride + m % slice_bytes, in 64 bits."""

def _index_desc_encode(
    desc: bytes, index: list[int], slice_bytes: int, stride: int
) -> bytes:
    """The FT_RTS_INDEXED payload around a descriptor of _RTS_DESC_BYTES."""

def _index_desc_decode(payload: bytes, size: int) -> tuple[list[int], int, int]:
    """(index, slice_bytes, stride) of a payload announcing `size` message
    bytes; ValueError for a malformed one."""

def _copy_index_sync(
    dst: int, dst_index: list[int] | None, dst_slice: int, dst_stride: int,
    src: int, src_index: list[int] | None, src_slice: int, src_stride: int,
    bytes: int, device: int, block_cap: int = 0, wide_index: bool = False,
) -> None:
    """One k_copy_indexed launch on raw device pointers, synchronous; None
    for a dense side. ValueError, before any device is touched, for two
    dense sides or slices that do not multiply out to `bytes`. wide_index
    runs the 64-bit index instantiation, which production takes only past
    2**32 - 1 granules."""

# Test hooks for the small-message kernels (csrc/smallmsg.hip). They call the
# host functions the engine calls; every wait has a host deadline of ~2 s.
# ValueError for a batch outside 1..32, a size above payload_max, seq 0 or a
# ring write out of range -- all checked before a device is touched.
class _InboxRing:
    """A ring from _inbox_ring_create (live), or geometry only when built
    here (detached: passes the argument checks, refused with RuntimeError by
    anything that needs device memory)."""

    def __init__(self, slots: int, slot_bytes: int) -> None: ...
    @property
    def slots(self) -> int: ...
    @property
    def slot_bytes(self) -> int: ...
    @property
    def hdr_bytes(self) -> int: ...
    @property
    def payload_max(self) -> int: ...
    @property
    def device(self) -> int: ...
    @property
    def live(self) -> bool: ...

class _InboxArmTicket: ...

def _inbox_ring_create(device: int) -> _InboxRing: ...
def _inbox_ring_destroy(ring: _InboxRing) -> None: ...
def _inbox_ring_read(ring: _InboxRing) -> bytes:
    """Device-to-host copy of the whole ring."""

def _inbox_ring_write(ring: _InboxRing, offset: int, data: bytes) -> None: ...
def _inbox_push_sync(
    ring: _InboxRing, msgs: list[tuple[int, int, int, int]], run_device: int
) -> None:
    """One k_inbox_push launch over (src_ptr, size, seq, tag) descriptors,
    polled to completion."""

def _inbox_unpack_sync(
    ring: _InboxRing, msgs: list[tuple[int, int, int]]
) -> list[tuple[int, bytes | None]]:
    """One k_inbox_unpack launch over (seq, size, dst_ptr or 0). Per
    message: status 1 (delivered) or 2 (payload never arrived within the
    kernel's spin bound), and the pinned bounce's `size` bytes when dst_ptr
    was 0, else None."""

def _inbox_arm_begin(
    ring: _InboxRing, expect_seq: int, tag: int, mask: int, dst: int,
    max_size: int, spin_iters: int = 0, precancel: bool = False,
) -> _InboxArmTicket:
    """Launch k_inbox_wait. spin_iters=0 is the process default. With
    precancel the cancel word is set before the launch is enqueued."""

def _inbox_arm_poll(ticket: _InboxArmTicket) -> tuple[int, int]:
    """(status, size): 0 running, 1 copied (`size` bytes), 2 nomatch,
    3 canceled, 4 expired."""

def _inbox_arm_cancel(ticket: _InboxArmTicket) -> None: ...
def _inbox_arm_end(ticket: _InboxArmTicket) -> tuple[int, int]:
    """Wait for a non-zero status, free the ticket, return (status, size).
    RuntimeError past the deadline; the pinned cell of a kernel that still
    has not reported is leaked, never reused."""

__version__: str
