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
    ) -> None: ...
    def recv(
        self,
        buffer: Buffer,
        tag: int,
        tag_mask: int,
        done_callback: Callable[[int, int], None],
        fail_callback: Callable[[str], None],
    ) -> None: ...
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
    ) -> None: ...
    def recv(
        self,
        buffer: Buffer,
        tag: int,
        tag_mask: int,
        done_callback: Callable[[int, int], None],
        fail_callback: Callable[[str], None],
    ) -> None: ...
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
def _copy_tuning() -> dict[str, int]: ...

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
) -> None:
    """Run the N-D copy kernels synchronously on raw device pointers
    (strides in bytes). path: "auto" (the production dispatch), "generic"
    (k_copy_nd) or "tiled" (k_copy_nd_tile; ValueError when the pair is not
    in the transpose family)."""

# k_copy_nd_tile tile extents: element bytes -> (T_A, T_B) in elements.
_ND_TILE: dict[int, tuple[int, int]]
_ND_MAX_DIMS: int

__version__: str
