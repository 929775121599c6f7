"""Python view of libsha1chunk.so -- the MI355X SHA-1 chunk engine.

Mirrors the reference's C hashing interface (same names, argument meaning and
error behaviour; file:line into /root/reference):

    shahash(data)                   chunk.c:35-51    one-shot SHA-1 -> 20 bytes
    binary2hex / hex2binary         chunk.c:57-85    lowercase hex codec
    make_chunks(path | file)        chunk.c:15-27    512 KiB chunk digests of a file
    get_chunk_hash(chunk)           chunk.c:168-185  hex digest (prints 2 lines)
    verify_hash(hex, data)          job.c:217-228    0 = match, 1 = mismatch
    verify_chunk_hash(path, hex, i) chunk.c:204-217  exit(-1) on mismatch
    SHA1()  .init/.update/.final    sha.h:58-60      streaming context

plus the batch / device entry points of include/sha1chunk.h that replace a
loop of shahash() calls.  The batch, device and verify-queue calls run on
the gfx950 HIP kernels; the reference's single-message calls (shahash,
get_chunk_hash, verify_hash, the SHA1 trio, make_chunks on a file of at most
4 MiB) hash on the host by default, as SURVEY.md 7.1 step 2 asks, and on the
kernels under SHA1CHUNK_HOST_SMALL=0 (include/sha1chunk.h, "Routing").  A
gfx950 device is required either way: there is no CPU fallback.  The library must have been built (`make -C
congestion-control-with-bittorren_amd` or __graft_entry__.build()); a missing
library or device raises, it never falls back.

PyTorch is only used for device memory and streams in the *_device helpers.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SHA1CHUNK_LIB selects another build of the library (the A/B build,
# `make ab` -> build-ab/libsha1chunk.so, for tools/sweep.py-style studies)
LIB_PATH = os.environ.get("SHA1CHUNK_LIB") or os.path.join(HERE, "libsha1chunk.so")
CHUNK_LEN = 524288  # constants.h:14
DIGEST_LEN = 20
SEED = 0x5EED0001

OK, EINVAL, ENODEV, ENOMEM, EHIP, EALIGN, EIO = 0, -1, -2, -3, -4, -5, -6
HOST, DEVICE, ALL_DEVICES = 0, 1, 2
NO_MATCH = 0xFFFFFFFF
KERNEL_AUTO, KERNEL_LANE, KERNEL_FUSED, KERNEL_SPLIT = 0, 1, 2, 3
KERNELS = {"auto": KERNEL_AUTO, "lane": KERNEL_LANE, "fused": KERNEL_FUSED, "split": KERNEL_SPLIT}


class Sha1ChunkError(RuntimeError):
    def __init__(self, code: int, where: str, msg: str):
        super().__init__(f"{where} failed ({code}): {msg}")
        self.code = code


class SHA1Context(C.Structure):
    """Same 96-byte layout as the reference SHA1Context (sha.h:39-52)."""
    _fields_ = [
        ("totalLength", C.c_uint64),
        ("hash", C.c_uint32 * 5),
        ("bufferLength", C.c_uint32),
        ("buffer", C.c_uint8 * 64),
    ]


_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p
READER_FN = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t)
SINK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, _u8p, C.c_size_t)

# (name, restype, argtypes) of every symbol the C ABI exports.
_SIGNATURES = [
    ("SHA1Init", None, [C.POINTER(SHA1Context)]),
    ("SHA1Update", None, [C.POINTER(SHA1Context), _vp, C.c_uint32]),
    ("SHA1Final", None, [C.POINTER(SHA1Context), _u8p]),
    ("shahash", None, [_u8p, C.c_int, _u8p]),
    ("binary2hex", None, [_u8p, C.c_int, C.c_char_p]),
    ("hex2binary", None, [C.c_char_p, C.c_int, _u8p]),
    ("make_chunks", C.c_int, [_vp, C.POINTER(_u8p)]),
    ("get_chunk_hash", C.c_void_p, [C.c_char_p, C.c_size_t]),
    ("verify_chunk_hash", None, [_vp, C.c_char_p, C.c_size_t]),
    ("verify_hash", C.c_int, [C.c_char_p, C.c_char_p]),
    # non-hash rest of chunk.h (csrc/chunk_file.c); read_chunk appends to the
    # peer's vector through the peer's vec_add, so it is called from C only
    ("read_chunk", None, [C.c_char_p, _vp]),
    ("find_chunk_idx_from_hash", C.c_size_t, [C.c_char_p, C.c_char_p]),
    ("seek_to_chunk_pos", None, [_vp, C.c_size_t]),
    ("seek_to_packet_pos", None, [_vp, C.c_size_t, C.c_size_t]),
    ("sha1chunk_hash_batch", C.c_int, [_vp, _u64p, _u32p, C.c_size_t, _u8p, C.c_uint]),
    ("sha1chunk_digest", C.c_int, [_vp, C.c_uint64, _u8p]),
    ("sha1chunk_verify_batch", C.c_int, [_vp, _u64p, _u32p, C.c_size_t, _u8p, _u8p, C.c_uint]),
    ("sha1chunk_hash_device_async", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_int]),
    ("sha1chunk_hash_uniform_async", C.c_int, [_vp, C.c_uint32, C.c_size_t, _vp, _vp, C.c_int]),
    ("sha1chunk_compare_device_async", C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    ("sha1chunk_hash_stream", C.c_long, [READER_FN, _vp, SINK_FN, _vp]),
    ("sha1chunk_hash_stream_sized", C.c_long, [READER_FN, _vp, SINK_FN, _vp, C.c_uint64]),
    ("sha1chunk_hash_fd", C.c_long, [C.c_int, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("sha1chunk_compress_blocks", C.c_int, [_u32p, _vp, C.c_size_t]),
    ("sha1chunk_finish", C.c_int, [_u32p, C.c_uint64, _vp, C.c_uint32, _u8p]),
    ("sha1chunk_synth_fill_async", C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, _vp]),
    ("sha1chunk_synth_fill_ragged_async", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp]),
    ("sha1chunk_vq_create", C.c_void_p, [C.c_size_t, C.c_uint32]),
    ("sha1chunk_vq_submit", C.c_int, [_vp, _vp, C.c_uint32, _u8p, C.c_uint64]),
    ("sha1chunk_vq_reserve", C.c_void_p, [_vp, C.c_uint32]),
    ("sha1chunk_vq_commit", C.c_int, [_vp, _vp, C.c_uint32, _u8p, C.c_uint64]),
    ("sha1chunk_vq_release", C.c_int, [_vp, _vp]),
    ("sha1chunk_vq_flush", C.c_int, [_vp]),
    ("sha1chunk_vq_poll", C.c_long, [_vp, _u64p, _u8p, C.c_size_t, C.c_int]),
    ("sha1chunk_vq_pending", C.c_size_t, [_vp]),
    ("sha1chunk_vq_destroy", None, [_vp]),
    ("sha1chunk_pv_create", C.c_void_p, [C.c_size_t, C.c_uint32]),
    ("sha1chunk_pv_open", C.c_void_p, [_vp, C.c_uint32, _u8p, C.c_uint64]),
    ("sha1chunk_pv_advance", C.c_int, [_vp, _vp, C.c_uint32]),
    ("sha1chunk_pv_hashed", C.c_int, [_vp, _vp, _u32p]),
    ("sha1chunk_pv_poll", C.c_long, [_vp, _u64p, _u8p, _u8p, C.c_size_t, C.c_int]),
    ("sha1chunk_pv_close", C.c_int, [_vp, _vp]),
    ("sha1chunk_pv_pending", C.c_size_t, [_vp]),
    ("sha1chunk_pv_destroy", None, [_vp]),
    ("sha1chunk_burst_advance", C.c_int, [_vp, C.POINTER(_vp), _u32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("sha1chunk_progress_stats", C.c_int, [_vp, _vp, C.c_size_t]),
    ("sha1chunk_init_device_async", C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    ("sha1chunk_update_device_async", C.c_int, [_vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    ("sha1chunk_final_device_async", C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp]),
    ("sha1chunk_update_batch", C.c_int, [_vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, C.c_uint]),
    ("sha1chunk_final_batch", C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_uint]),
    ("sha1chunk_pinned_alloc", C.c_void_p, [C.c_size_t]),
    ("sha1chunk_pinned_free", C.c_int, [_vp]),
    ("sha1chunk_gather_device_async", C.c_int,
     [_vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, C.c_uint64, _vp, _vp]),
    ("sha1chunk_hash_gather_batch", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_uint]),
    ("sha1chunk_verify_gather_batch", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, C.c_uint]),
    ("sha1chunk_index_create", C.c_void_p, [_vp, C.c_size_t, C.c_uint]),
    ("sha1chunk_index_destroy", None, [_vp]),
    ("sha1chunk_index_size", C.c_size_t, [_vp]),
    ("sha1chunk_index_lookup_device_async", C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    ("sha1chunk_index_lookup", C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    ("sha1chunk_index_reserve", C.c_int, [_vp, C.c_size_t]),
    ("sha1chunk_index_capacity", C.c_size_t, [_vp]),
    ("sha1chunk_index_append_device_async", C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    ("sha1chunk_index_append", C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    ("sha1chunk_admit_batch", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_uint]),
    ("sha1chunk_match_batch", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_uint]),
    ("sha1chunk_match_fd", C.c_long, [_vp, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("sha1chunk_device_count", C.c_int, []),
    ("sha1chunk_set_device", C.c_int, [C.c_int]),
    ("sha1chunk_get_device", C.c_int, []),
    ("sha1chunk_device_pci_bus_id", C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    ("sha1chunk_receive_cpus", C.c_int, [C.c_int, C.c_uint, _vp, C.c_size_t, C.POINTER(C.c_uint)]),
    ("sha1chunk_last_error", C.c_char_p, []),
    ("sha1chunk_version", C.c_char_p, []),
]


class ProgressStats(C.Structure):
    """sha1chunk_progress_stats_t (include/sha1chunk.h)."""
    _fields_ = [
        ("launches", C.c_uint64),
        ("launches_shared", C.c_uint64),
        ("entries", C.c_uint64),
        ("blocks", C.c_uint64),
        ("kernel", C.c_uint32),
        ("depth", C.c_uint32),
    ]


_lib: C.CDLL | None = None


def _one_hip_runtime() -> None:
    """One HIP runtime per process.  The library's backend binds to the HIP
    runtime already loaded in the process (same soname); loaded before
    PyTorch's, it brings /opt/rocm's own and the process then holds two, and
    torch sees no device (tools/order_probe.py, profiles/order_probe_r06.log).
    So where PyTorch is installed it is imported first, which maps its
    runtime without starting it (the host-routed calls still never open
    /dev/kfd: tests/test_host_small.py).  A PyTorch that is installed but
    fails to import (OSError for a missing shared object, RuntimeError) is as
    good as none: the library then brings its own runtime, and the host-only
    calls (binary2hex ...) need none at all."""
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001 -- whatever a broken install raises
        pass


def lib() -> C.CDLL:
    """Load libsha1chunk.so (raises if it was never built)."""
    global _lib
    if _lib is None:
        _one_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: build it with __graft_entry__.build() or "
                "`make -C congestion-control-with-bittorren_amd`")
        L = C.CDLL(LIB_PATH)
        for name, res, args in _SIGNATURES:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        L.free = C.CDLL(None).free
        L.free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def exported_symbols() -> list[str]:
    return [s[0] for s in _SIGNATURES]


def _check(rc: int, where: str) -> int:
    if rc < 0:
        raise Sha1ChunkError(rc, where, lib().sha1chunk_last_error().decode(errors="replace"))
    return rc


def _np_ptr(a: np.ndarray, t=_u8p):
    return a.ctypes.data_as(t)


# ------------------------------------------------------------ device mgmt --
def device_count() -> int:
    n = lib().sha1chunk_device_count()
    return max(n, 0)


def set_device(dev: int) -> None:
    _check(lib().sha1chunk_set_device(dev), "sha1chunk_set_device")


def device_pci_bus_id(dev: int) -> str:
    """PCI address of logical device `dev`'s physical GPU."""
    buf = C.create_string_buffer(64)
    _check(lib().sha1chunk_device_pci_bus_id(dev, buf, len(buf)), "sha1chunk_device_pci_bus_id")
    return buf.value.decode()


def receive_cpus(dev: int, slot: int) -> tuple[list[int], int]:
    """The CPUs for receive thread `slot` of a verify queue on `dev` (one L3
    domain of the device's NUMA node) and the number of such domains."""
    mask = (C.c_uint8 * 128)()  # a glibc cpu_set_t: 1024 CPUs
    doms = C.c_uint(0)
    _check(lib().sha1chunk_receive_cpus(dev, slot, mask, len(mask), C.byref(doms)), "sha1chunk_receive_cpus")
    return [8 * i + b for i in range(len(mask)) for b in range(8) if mask[i] >> b & 1], doms.value


def version() -> str:
    return lib().sha1chunk_version().decode()


# ------------------------------------------------- reference-named API ----
def binary2hex(buf: bytes) -> str:
    """chunk.c:57-63 -- lowercase hex of buf."""
    b = np.frombuffer(bytes(buf) + b"\0", np.uint8)
    out = C.create_string_buffer(2 * len(buf) + 1)
    lib().binary2hex(_np_ptr(b), len(buf), out)
    return out.value.decode()


def hex2binary(hexstr: str) -> bytes:
    """chunk.c:78-85 -- hex (either case) to bytes."""
    raw = hexstr.encode()
    out = np.zeros(max(len(raw) // 2, 1), np.uint8)
    lib().hex2binary(raw, len(raw), _np_ptr(out))
    return out[: len(raw) // 2].tobytes()


def shahash(data: bytes | np.ndarray) -> bytes:
    """chunk.c:35-51 -- SHA-1 of one message (sha1chunk_digest: on the host
    by default, on the kernels under SHA1CHUNK_HOST_SMALL=0; a device is
    required either way).  Raises instead of exit(-1)."""
    buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else \
        np.ascontiguousarray(data, np.uint8).reshape(-1)
    n = buf.size
    if n == 0:
        buf = np.zeros(1, np.uint8)
    out = np.zeros(DIGEST_LEN, np.uint8)
    _check(lib().sha1chunk_digest(buf.ctypes.data, n, _np_ptr(out)), "shahash")
    return out.tobytes()


def get_chunk_hash(chunk: bytes) -> str:
    """chunk.c:168-185 -- hex digest; the C side prints the reference's two lines."""
    p = lib().get_chunk_hash(bytes(chunk), len(chunk))
    try:
        return C.string_at(p).decode()
    finally:
        lib().free(p)


def verify_hash(chunk_hash: str, data: bytes) -> int:
    """job.c:217-228 -- hashes CHUNK_LEN bytes of data; 0 = match, 1 = mismatch."""
    buf = bytes(data)
    if len(buf) < CHUNK_LEN:
        raise ValueError("verify_hash reads CHUNK_LEN (524288) bytes of data")
    return lib().verify_hash(chunk_hash.encode(), buf)


def make_chunks(src) -> list[bytes]:
    """chunk.c:15-27 -- digests of every 512 KiB chunk of a file (path or
    binary file object opened on a real fd)."""
    if isinstance(src, (str, os.PathLike)):
        with open(src, "rb") as f:
            return make_chunks(f)
    fd = src.fileno()
    pos = src.tell()
    os.lseek(fd, pos, os.SEEK_SET)
    size = os.fstat(fd).st_size - pos
    cap = max((size + CHUNK_LEN - 1) // CHUNK_LEN, 1)
    out = np.zeros((cap, DIGEST_LEN), np.uint8)
    total = C.c_size_t(0)
    n = _check(lib().sha1chunk_hash_fd(fd, _np_ptr(out), cap, C.byref(total)), "make_chunks")
    if total.value > cap:
        raise Sha1ChunkError(EIO, "make_chunks", "file grew while hashing")
    return [out[i].tobytes() for i in range(n)]


class SHA1:
    """sha.h:58-60 streaming context (SHA1Init / SHA1Update / SHA1Final)."""

    def __init__(self):
        self.ctx = SHA1Context()
        lib().SHA1Init(C.byref(self.ctx))

    def update(self, data: bytes) -> "SHA1":
        b = bytes(data)
        lib().SHA1Update(C.byref(self.ctx), b, len(b))
        return self

    def final(self) -> bytes:
        out = np.zeros(DIGEST_LEN, np.uint8)
        lib().SHA1Final(C.byref(self.ctx), _np_ptr(out))
        return out.tobytes()


# ------------------------------------------------------------- batch API --
def hash_batch(base: np.ndarray | bytes, offsets: Sequence[int], lengths: Sequence[int],
               all_devices: bool = False) -> np.ndarray:
    """digests[i] = SHA-1(base[offsets[i]:offsets[i]+lengths[i]]) -> (n, 20) uint8."""
    b = np.frombuffer(base, np.uint8) if isinstance(base, (bytes, bytearray)) else \
        np.ascontiguousarray(base).view(np.uint8).reshape(-1)
    if b.size == 0:
        b = np.zeros(1, np.uint8)
    off = np.ascontiguousarray(offsets, np.uint64)
    ln = np.ascontiguousarray(lengths, np.uint32)
    if off.shape != ln.shape:
        raise ValueError("offsets and lengths differ in length")
    if off.size and int((off + ln).max()) > (b.size if len(base) else 0):
        raise ValueError("chunk range outside the buffer")
    out = np.zeros((off.size, DIGEST_LEN), np.uint8)
    flags = ALL_DEVICES if all_devices else HOST
    _check(lib().sha1chunk_hash_batch(b.ctypes.data, _np_ptr(off, _u64p), _np_ptr(ln, _u32p),
                                      off.size, _np_ptr(out), flags), "sha1chunk_hash_batch")
    return out


def verify_batch(base, offsets, lengths, expected: np.ndarray, all_devices: bool = False) -> np.ndarray:
    """verify_hash() semantics per chunk: 0 = match, 1 = mismatch."""
    b = np.ascontiguousarray(np.frombuffer(base, np.uint8) if isinstance(base, (bytes, bytearray))
                             else base).view(np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, np.uint64)
    ln = np.ascontiguousarray(lengths, np.uint32)
    exp = np.ascontiguousarray(expected, np.uint8).reshape(-1, DIGEST_LEN)
    mism = np.zeros(off.size, np.uint8)
    flags = ALL_DEVICES if all_devices else HOST
    _check(lib().sha1chunk_verify_batch(b.ctypes.data, _np_ptr(off, _u64p), _np_ptr(ln, _u32p),
                                        off.size, _np_ptr(exp), _np_ptr(mism), flags),
           "sha1chunk_verify_batch")
    return mism


class Reservation:
    """A buffer handed out by VerifyQueue.reserve(): `view` is a writable
    uint8 array over it (valid until the queue releases it)."""

    def __init__(self, ptr: int, length: int):
        self.ptr = ptr
        self.length = length
        self.view = np.ctypeslib.as_array(C.cast(ptr, _u8p), shape=(max(length, 1),))[:length]


class VerifyQueue:
    """Asynchronous batched verify for the peer's receive path: the batched
    counterpart of verify_hash() (job.c:217-228).  submit() stages a chunk
    with its expected digest and a tag; poll() yields (tag, mismatch) with
    mismatch 0 = match, 1 = mismatch (re-GET), as verify_hash returns."""

    def __init__(self, batch: int = 256, max_chunk_len: int = CHUNK_LEN):
        self._q = lib().sha1chunk_vq_create(batch, max_chunk_len)
        if not self._q:
            raise Sha1ChunkError(ENODEV if device_count() == 0 else EINVAL, "sha1chunk_vq_create",
                                 lib().sha1chunk_last_error().decode(errors="replace"))

    def submit(self, chunk: bytes, expected: bytes | str, tag: int) -> None:
        exp = bytes.fromhex(expected) if isinstance(expected, str) else bytes(expected)
        if len(exp) != DIGEST_LEN:
            raise ValueError("expected digest must be 20 bytes / 40 hex chars")
        e = np.frombuffer(exp, np.uint8)
        b = bytes(chunk)
        _check(lib().sha1chunk_vq_submit(self._q, b, len(b), _np_ptr(e), tag), "sha1chunk_vq_submit")

    def reserve(self, length: int) -> "Reservation":
        """A buffer of `length` bytes inside the queue (the peer's session
        buffer, reliable_udp.c:121): fill `.view` in place, then commit()."""
        p = lib().sha1chunk_vq_reserve(self._q, length)
        if not p:
            raise Sha1ChunkError(ENOMEM, "sha1chunk_vq_reserve",
                                 lib().sha1chunk_last_error().decode(errors="replace"))
        return Reservation(p, length)

    def commit(self, r: "Reservation", expected: bytes | str, tag: int, length: int | None = None) -> None:
        """Verify a filled reservation where it lies (packet_handler.c:472)."""
        exp = bytes.fromhex(expected) if isinstance(expected, str) else bytes(expected)
        if len(exp) != DIGEST_LEN:
            raise ValueError("expected digest must be 20 bytes / 40 hex chars")
        e = np.frombuffer(exp, np.uint8)
        n = r.length if length is None else length
        _check(lib().sha1chunk_vq_commit(self._q, r.ptr, n, _np_ptr(e), tag), "sha1chunk_vq_commit")

    def release(self, r: "Reservation") -> None:
        """Give a reservation back (after its result, or instead of a commit)."""
        _check(lib().sha1chunk_vq_release(self._q, r.ptr), "sha1chunk_vq_release")

    def flush(self) -> None:
        _check(lib().sha1chunk_vq_flush(self._q), "sha1chunk_vq_flush")

    def poll(self, wait: bool = False, max_results: int = 1 << 16) -> list[tuple[int, int]]:
        tags = np.zeros(max_results, np.uint64)
        mism = np.zeros(max_results, np.uint8)
        n = _check(lib().sha1chunk_vq_poll(self._q, _np_ptr(tags, _u64p), _np_ptr(mism), max_results,
                                           1 if wait else 0), "sha1chunk_vq_poll")
        return [(int(tags[i]), int(mism[i])) for i in range(n)]

    @property
    def pending(self) -> int:
        return int(lib().sha1chunk_vq_pending(self._q))

    def close(self) -> None:
        if self._q:
            lib().sha1chunk_vq_destroy(self._q)
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProgressiveVerifier:
    """Verify chunks while they are received (sha1chunk_pv, include/
    sha1chunk.h): open() hands out a session's buffer -- the peer's
    recv_session->data -- as a `Reservation`; advance(r, ready) states that
    bytes [0, ready) are final (after cumulative_ack: min(len, 1484 *
    last_packet_acked)) and the device hashes them while the rest arrives;
    poll() yields (tag, mismatch) as verify_hash returns it, with the
    computed digests too under with_digests=True."""

    def __init__(self, sessions: int = 64, max_chunk_len: int = CHUNK_LEN):
        self._p = lib().sha1chunk_pv_create(sessions, max_chunk_len)
        if not self._p:
            raise Sha1ChunkError(ENODEV if device_count() == 0 else EINVAL, "sha1chunk_pv_create",
                                 lib().sha1chunk_last_error().decode(errors="replace"))

    def open(self, length: int, expected: bytes | str, tag: int) -> "Reservation":
        """A session for a chunk of `length` bytes: fill `.view` in place."""
        exp = bytes.fromhex(expected) if isinstance(expected, str) else bytes(expected)
        if len(exp) != DIGEST_LEN:
            raise ValueError("expected digest must be 20 bytes / 40 hex chars")
        e = np.frombuffer(exp, np.uint8)
        p = lib().sha1chunk_pv_open(self._p, length, _np_ptr(e), tag)
        if not p:
            raise Sha1ChunkError(ENOMEM, "sha1chunk_pv_open",
                                 lib().sha1chunk_last_error().decode(errors="replace"))
        return Reservation(p, length)

    def advance(self, r: "Reservation", ready: int) -> None:
        """Bytes [0, ready) of the session are final; ready == length completes it."""
        _check(lib().sha1chunk_pv_advance(self._p, r.ptr, ready), "sha1chunk_pv_advance")

    def advance_many(self, pairs) -> int:
        """advance() for every (reservation, ready) of `pairs`, in order, in
        one call (sha1chunk_burst_advance): one lock, one launch decision.
        Returns the number applied; a refused pair raises, with the pairs
        before it applied and their count in the error's `.applied`."""
        pairs = list(pairs)
        n = len(pairs)
        bufs = (_vp * max(n, 1))(*[r.ptr for r, _ in pairs])
        marks = (C.c_uint32 * max(n, 1))(*[ready for _, ready in pairs])
        applied = C.c_size_t(0)
        rc = lib().sha1chunk_burst_advance(self._p, bufs, marks, n, C.byref(applied))
        if rc < 0:
            err = Sha1ChunkError(rc, "sha1chunk_burst_advance",
                                 lib().sha1chunk_last_error().decode(errors="replace"))
            err.applied = applied.value
            raise err
        return applied.value

    def stats(self) -> dict:
        """The object's launch counters (sha1chunk_progress_stats): launches,
        launches_shared, entries, blocks, kernel ("auto" / "lane" /
        "shared") and depth."""
        st = ProgressStats()
        _check(lib().sha1chunk_progress_stats(self._p, C.byref(st), C.sizeof(st)), "sha1chunk_progress_stats")
        return {"launches": st.launches, "launches_shared": st.launches_shared, "entries": st.entries,
                "blocks": st.blocks, "kernel": ("auto", "lane", "shared")[st.kernel], "depth": st.depth}

    def hashed(self, r: "Reservation") -> int:
        """Bytes of the session the device has confirmed hashed."""
        n = C.c_uint32(0)
        _check(lib().sha1chunk_pv_hashed(self._p, r.ptr, C.byref(n)), "sha1chunk_pv_hashed")
        return n.value

    def poll(self, wait: bool = False, max_results: int = 1 << 12, with_digests: bool = False):
        """Finished [(tag, mismatch)], or [(tag, mismatch, digest)] with_digests."""
        tags = np.zeros(max_results, np.uint64)
        mism = np.zeros(max_results, np.uint8)
        dig = np.zeros((max_results, DIGEST_LEN), np.uint8) if with_digests else None
        n = _check(lib().sha1chunk_pv_poll(self._p, _np_ptr(tags, _u64p), _np_ptr(mism),
                                           _np_ptr(dig) if with_digests else None, max_results,
                                           1 if wait else 0), "sha1chunk_pv_poll")
        if with_digests:
            return [(int(tags[i]), int(mism[i]), dig[i].tobytes()) for i in range(n)]
        return [(int(tags[i]), int(mism[i])) for i in range(n)]

    def close(self, r: "Reservation") -> None:
        """Free a session: before completion (dropped) or after its result."""
        _check(lib().sha1chunk_pv_close(self._p, r.ptr), "sha1chunk_pv_close")

    @property
    def pending(self) -> int:
        return int(lib().sha1chunk_pv_pending(self._p))

    def destroy(self) -> None:
        if self._p:
            lib().sha1chunk_pv_destroy(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ------------------------------------------------------ device (torch) ----
def _stream_ptr(stream) -> int | None:
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def hash_device(base, offsets, lengths, digests, stream=None, kernel: int | str = KERNEL_AUTO) -> None:
    """Enqueue the hash of a device-resident batch (torch CUDA tensors:
    base uint8, offsets int64, lengths int32, digests uint8 (n, 20))."""
    k = KERNELS[kernel] if isinstance(kernel, str) else kernel
    n = offsets.numel()
    _check(lib().sha1chunk_hash_device_async(base.data_ptr(), offsets.data_ptr(), lengths.data_ptr(),
                                             n, digests.data_ptr(), _stream_ptr(stream), k),
           "sha1chunk_hash_device_async")


def hash_uniform_device(base, chunk_len: int, n: int, digests, stream=None,
                        kernel: int | str = KERNEL_AUTO) -> None:
    k = KERNELS[kernel] if isinstance(kernel, str) else kernel
    _check(lib().sha1chunk_hash_uniform_async(base.data_ptr(), chunk_len, n, digests.data_ptr(),
                                              _stream_ptr(stream), k),
           "sha1chunk_hash_uniform_async")


def compare_device(digests, expected, mismatch, stream=None) -> None:
    _check(lib().sha1chunk_compare_device_async(digests.data_ptr(), expected.data_ptr(),
                                                mismatch.numel(), mismatch.data_ptr(),
                                                _stream_ptr(stream)),
           "sha1chunk_compare_device_async")


def _dev_ptr(t, ctype):
    """A device tensor's address (or a plain int) as the ctypes pointer type
    a host/device entry point is declared with."""
    return C.cast(C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t)), ctype)


def hash_batch_device(base, offsets, lengths, digests, n: int | None = None) -> None:
    """sha1chunk_hash_batch(..., SHA1CHUNK_DEVICE): every buffer a tensor on
    the current device (or a raw address).  Synchronous: the digests are in
    `digests` when the call returns."""
    n = offsets.numel() if n is None else n
    _check(lib().sha1chunk_hash_batch(_dev_ptr(base, _vp), _dev_ptr(offsets, _u64p), _dev_ptr(lengths, _u32p), n,
                                      _dev_ptr(digests, _u8p), DEVICE), "sha1chunk_hash_batch")


def verify_batch_device(base, offsets, lengths, expected, mismatch, n: int | None = None) -> None:
    """sha1chunk_verify_batch(..., SHA1CHUNK_DEVICE): `expected` (n x 20) and
    `mismatch` (n bytes) are device buffers too.  Synchronous."""
    n = offsets.numel() if n is None else n
    _check(lib().sha1chunk_verify_batch(_dev_ptr(base, _vp), _dev_ptr(offsets, _u64p), _dev_ptr(lengths, _u32p), n,
                                        _dev_ptr(expected, _u8p), _dev_ptr(mismatch, _u8p), DEVICE),
           "sha1chunk_verify_batch")


# ---- batched SHA1Init / SHA1Update / SHA1Final over arrays of SHA1Context ----
CONTEXT_BYTES = 96
CONTEXT_DTYPE = np.dtype([("totalLength", "<u8"), ("hash", "<u4", (5,)), ("bufferLength", "<u4"),
                          ("buffer", "u1", (64,))])


def _addr(x) -> int | None:
    """Address of a torch tensor, a numpy array or a plain int (None stays None)."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return int(x)


def _count(contexts, n_contexts: int | None) -> int:
    if n_contexts is not None:
        return n_contexts
    nbytes = contexts.numel() * contexts.element_size() if hasattr(contexts, "numel") else contexts.nbytes
    return nbytes // CONTEXT_BYTES


def init_contexts_device(contexts, index=None, n: int | None = None, n_contexts: int | None = None,
                         stream=None) -> None:
    """Enqueue SHA1Init of the listed contexts (a device buffer of 96-byte
    structs; index: device uint32/int32 tensor or None for contexts 0..n-1)."""
    nc = _count(contexts, n_contexts)
    n = (index.numel() if index is not None else nc) if n is None else n
    _check(lib().sha1chunk_init_device_async(_addr(contexts), nc, _addr(index), n, _stream_ptr(stream)),
           "sha1chunk_init_device_async")


def update_contexts_device(contexts, base, offsets, lengths, index=None, n: int | None = None,
                           n_contexts: int | None = None, stream=None) -> None:
    """Enqueue SHA1Update(&contexts[index[i]], base + offsets[i], lengths[i])
    for every entry (torch CUDA tensors: offsets int64, lengths int32)."""
    nc = _count(contexts, n_contexts)
    n = offsets.numel() if n is None else n
    _check(lib().sha1chunk_update_device_async(_addr(contexts), nc, _addr(index), _addr(base), _addr(offsets),
                                               _addr(lengths), n, _stream_ptr(stream)),
           "sha1chunk_update_device_async")


def final_contexts_device(contexts, digests=None, index=None, n: int | None = None, n_contexts: int | None = None,
                          stream=None) -> None:
    """Enqueue SHA1Final of the listed contexts; digests (n, 20) uint8 on the
    device, or None."""
    nc = _count(contexts, n_contexts)
    n = (index.numel() if index is not None else nc) if n is None else n
    _check(lib().sha1chunk_final_device_async(_addr(contexts), nc, _addr(index), n, _addr(digests),
                                              _stream_ptr(stream)), "sha1chunk_final_device_async")


def new_contexts(n: int) -> np.ndarray:
    """n host contexts as SHA1Init leaves them (a CONTEXT_DTYPE array)."""
    ctx = np.zeros(n, CONTEXT_DTYPE)
    ctx["hash"] = np.array([0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0], np.uint32)
    return ctx


def update_batch(contexts: np.ndarray, base, offsets, lengths, index=None) -> None:
    """sha1chunk_update_batch(..., SHA1CHUNK_HOST): contexts is a writable
    host array of 96-byte structs (CONTEXT_DTYPE), updated in place."""
    b = np.frombuffer(base, np.uint8) if isinstance(base, (bytes, bytearray)) else \
        np.ascontiguousarray(base).view(np.uint8).reshape(-1)
    if b.size == 0:
        b = np.zeros(1, np.uint8)
    off = np.ascontiguousarray(offsets, np.uint64)
    ln = np.ascontiguousarray(lengths, np.uint32)
    if off.shape != ln.shape:
        raise ValueError("offsets and lengths differ in length")
    idx = None if index is None else np.ascontiguousarray(index, np.uint32)
    if idx is not None and idx.shape != ln.shape:
        raise ValueError("index and lengths differ in length")
    _check(lib().sha1chunk_update_batch(contexts.ctypes.data, _count(contexts, None), _addr(idx), b.ctypes.data,
                                        off.ctypes.data, ln.ctypes.data, off.size, HOST), "sha1chunk_update_batch")


def final_batch(contexts: np.ndarray, index=None) -> np.ndarray:
    """sha1chunk_final_batch(..., SHA1CHUNK_HOST) -> (n, 20) uint8 digests;
    the contexts are left as SHA1Final leaves them."""
    idx = None if index is None else np.ascontiguousarray(index, np.uint32)
    nc = _count(contexts, None)
    n = nc if idx is None else idx.size
    out = np.zeros((n, DIGEST_LEN), np.uint8)
    _check(lib().sha1chunk_final_batch(contexts.ctypes.data, nc, _addr(idx), n, out.ctypes.data, HOST),
           "sha1chunk_final_batch")
    return out


# ---- messages given as segment lists (device gather) ----
def pinned_alloc(nbytes: int) -> np.ndarray:
    """sha1chunk_pinned_alloc: nbytes of pinned host memory the device reads in
    place (a packet ring), as a uint8 numpy view.  The view does not own the
    memory: hand it (or its address) to pinned_free when done, and use no view
    of it afterwards."""
    p = lib().sha1chunk_pinned_alloc(nbytes)
    if not p:
        raise Sha1ChunkError(ENOMEM, "sha1chunk_pinned_alloc", lib().sha1chunk_last_error().decode(errors="replace"))
    return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p))


def pinned_free(buf) -> None:
    """sha1chunk_pinned_free of a pinned_alloc view (or its address)."""
    _check(lib().sha1chunk_pinned_free(_addr(buf)), "sha1chunk_pinned_free")


def segment_csr(messages) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The CSR segment list (seg_offsets uint64, seg_lengths uint32, seg_first
    uint32 of n + 1 entries) of a list of per-message [(offset, length), ...]
    lists.  A tuple of three arrays is taken as such a list already."""
    if isinstance(messages, tuple) and len(messages) == 3 and all(isinstance(a, np.ndarray) for a in messages):
        off, ln, first = messages
        return (np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(ln, np.uint32),
                np.ascontiguousarray(first, np.uint32))
    first = np.zeros(len(messages) + 1, np.uint32)
    first[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    flat = np.array([seg for m in messages for seg in m], np.uint64).reshape(-1, 2)
    return np.ascontiguousarray(flat[:, 0]), flat[:, 1].astype(np.uint32), first


def gather_device(base, seg_offsets, seg_lengths, seg_first, dst, dst_offsets, out_lengths=None, n: int | None = None,
                  n_segments: int | None = None, dst_bytes: int | None = None, stream=None) -> None:
    """Enqueue sha1chunk_gather_device_async: message i, the concatenation of
    segments seg_first[i] .. seg_first[i+1]-1 (segment s = seg_lengths[s] bytes
    at base + seg_offsets[s]), is written at dst + dst_offsets[i].  Torch CUDA
    tensors (offsets int64, lengths / seg_first / out_lengths int32); base may
    also be a pinned_alloc view."""
    n = seg_first.numel() - 1 if n is None else n
    n_segments = seg_lengths.numel() if n_segments is None else n_segments
    dst_bytes = dst.numel() * dst.element_size() if dst_bytes is None else dst_bytes
    _check(lib().sha1chunk_gather_device_async(_addr(base), _addr(seg_offsets), _addr(seg_lengths), n_segments,
                                               _addr(seg_first), n, _addr(dst), _addr(dst_offsets), dst_bytes,
                                               _addr(out_lengths), _stream_ptr(stream)),
           "sha1chunk_gather_device_async")


def _gather_base(base) -> tuple[int, int, object]:
    """(address, flags, keep-alive) of a gather source: a torch CUDA tensor is
    device memory, anything else host memory (pinned or pageable)."""
    if hasattr(base, "data_ptr"):
        return base.data_ptr(), DEVICE if base.is_cuda else HOST, base
    b = np.frombuffer(base, np.uint8) if isinstance(base, (bytes, bytearray)) else base
    if not b.flags["C_CONTIGUOUS"]:
        raise ValueError("gather source must be contiguous")
    return b.ctypes.data, HOST, b


def hash_gather(base, messages) -> np.ndarray:
    """sha1chunk_hash_gather_batch -> (n, 20) uint8 digests.  messages: a list
    of per-message [(offset, length), ...] lists (or segment_csr's tuple);
    base: a torch CUDA tensor, a pinned_alloc view or any host array."""
    off, ln, first = segment_csr(messages)
    addr, flags, _keep = _gather_base(base)
    out = np.zeros((first.size - 1, DIGEST_LEN), np.uint8)
    _check(lib().sha1chunk_hash_gather_batch(addr, off.ctypes.data, ln.ctypes.data, ln.size, first.ctypes.data,
                                             first.size - 1, out.ctypes.data, flags), "sha1chunk_hash_gather_batch")
    return out


def verify_gather(base, messages, expected) -> np.ndarray:
    """sha1chunk_verify_gather_batch -> n mismatch bytes (verify_hash's 0 / 1)
    against expected, (n, 20) uint8."""
    off, ln, first = segment_csr(messages)
    addr, flags, _keep = _gather_base(base)
    exp = np.ascontiguousarray(expected, np.uint8).reshape(-1)
    if exp.size != (first.size - 1) * DIGEST_LEN:
        raise ValueError("expected must hold 20 bytes per message")
    out = np.zeros(first.size - 1, np.uint8)
    _check(lib().sha1chunk_verify_gather_batch(addr, off.ctypes.data, ln.ctypes.data, ln.size, first.ctypes.data,
                                               first.size - 1, exp.ctypes.data, out.ctypes.data, flags),
           "sha1chunk_verify_gather_batch")
    return out


# ---- digest index: match chunk digests against a chunk list ----
def _digest_rows(digests) -> np.ndarray:
    """Host digests -- an (n, 20) uint8 array, or a sequence of 20-byte
    strings -- as one contiguous (n, 20) uint8 array."""
    if isinstance(digests, np.ndarray):
        a = np.ascontiguousarray(digests, np.uint8)
    else:
        a = np.frombuffer(b"".join(bytes(d) for d in digests), np.uint8)
    if a.size % DIGEST_LEN:
        raise ValueError("digests must hold 20 bytes each")
    return a.reshape(-1, DIGEST_LEN)


class DigestIndex:
    """A set of m known digests on the device, queried with digests and
    answering with positions (sha1chunk_index, include/sha1chunk.h): digest p
    of `digests` has position p, a lookup gives the lowest position that holds
    a queried digest or NO_MATCH.  `digests`: an (m, 20) uint8 array or a
    sequence of 20-byte strings in host memory, or a torch CUDA uint8 tensor
    (complete before the call) with m given or taken from its size.  The index
    belongs to the device current at the call.  The set grows by `append`,
    `append_device` and `admit_batch`: digest i of a call gets position
    size + i, and a digest whose skip byte is set uses its position up without
    joining the set."""

    def __init__(self, digests, m: int | None = None):
        if hasattr(digests, "data_ptr"):
            keep, flags = digests, DEVICE if digests.is_cuda else HOST
            m = digests.numel() * digests.element_size() // DIGEST_LEN if m is None else m
            addr = digests.data_ptr()
        else:
            keep, flags = _digest_rows(digests), HOST
            m = keep.shape[0] if m is None else m
            addr = keep.ctypes.data
        self._ix = lib().sha1chunk_index_create(addr if m else None, m, flags)
        del keep  # the index owns a copy
        if not self._ix:
            raise Sha1ChunkError(ENODEV if device_count() == 0 else EINVAL, "sha1chunk_index_create",
                                 lib().sha1chunk_last_error().decode(errors="replace"))

    @property
    def size(self) -> int:
        return int(lib().sha1chunk_index_size(self._ix))

    def __len__(self) -> int:
        return self.size

    @property
    def capacity(self) -> int:
        return int(lib().sha1chunk_index_capacity(self._ix))

    def reserve(self, capacity: int) -> None:
        """sha1chunk_index_reserve: room for at least `capacity` digests."""
        _check(lib().sha1chunk_index_reserve(self._ix, capacity), "sha1chunk_index_reserve")

    def append(self, digests, skip=None) -> int:
        """sha1chunk_index_append of host digests (skip: one byte per digest,
        non-zero = not admitted, or None) -> the position of the first; grows
        the index when it is full."""
        q = _digest_rows(digests)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(-1)
        if sk is not None and sk.size != q.shape[0]:
            raise ValueError("digests and skip differ in length")
        first = self.size
        _check(lib().sha1chunk_index_append(self._ix, q.ctypes.data, q.shape[0], None if sk is None else sk.ctypes.data),
               "sha1chunk_index_append")
        return first

    def append_device(self, digests, k: int | None = None, skip=None, stream=None) -> int:
        """Enqueue sha1chunk_index_append_device_async: digests a torch CUDA
        uint8 tensor of k x 20 bytes, skip one of k bytes or None -> the
        position of the first.  Never grows: reserve first."""
        k = digests.numel() * digests.element_size() // DIGEST_LEN if k is None else k
        first = self.size
        _check(lib().sha1chunk_index_append_device_async(self._ix, _addr(digests), k, _addr(skip), _stream_ptr(stream)),
               "sha1chunk_index_append_device_async")
        return first

    def admit_batch(self, base, offsets, lengths, expected, mismatch=None):
        """sha1chunk_admit_batch: verify every chunk against its expected
        digest and append all digests with skip = mismatch, so that exactly the
        verified chunks join the set.  Host form (base bytes or a numpy array,
        offsets and lengths sequences, expected host digests) -> n mismatch
        bytes; device form (torch CUDA tensors: base uint8, offsets int64,
        lengths int32, expected uint8, and mismatch uint8 to receive the
        verdicts) -> mismatch."""
        if hasattr(base, "data_ptr"):
            if mismatch is None:
                raise ValueError("the device form needs a mismatch tensor")
            _check(lib().sha1chunk_admit_batch(self._ix, _addr(base), _addr(offsets), _addr(lengths), offsets.numel(),
                                               _addr(expected), _addr(mismatch), DEVICE), "sha1chunk_admit_batch")
            return mismatch
        b = np.frombuffer(base, np.uint8) if isinstance(base, (bytes, bytearray)) else \
            np.ascontiguousarray(base).view(np.uint8).reshape(-1)
        if b.size == 0:
            b = np.zeros(1, np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        ln = np.ascontiguousarray(lengths, np.uint32)
        exp = _digest_rows(expected)
        if off.shape != ln.shape or exp.shape[0] != off.size:
            raise ValueError("offsets, lengths and expected differ in length")
        out = np.zeros(off.size, np.uint8)
        _check(lib().sha1chunk_admit_batch(self._ix, b.ctypes.data, off.ctypes.data, ln.ctypes.data, off.size,
                                           exp.ctypes.data, out.ctypes.data, HOST), "sha1chunk_admit_batch")
        return out

    def lookup(self, digests) -> np.ndarray:
        """sha1chunk_index_lookup of host digests -> n uint32 positions."""
        q = _digest_rows(digests)
        ids = np.full(q.shape[0], NO_MATCH, np.uint32)
        _check(lib().sha1chunk_index_lookup(self._ix, q.ctypes.data, q.shape[0], ids.ctypes.data),
               "sha1chunk_index_lookup")
        return ids

    def lookup_device(self, digests, ids, n: int | None = None, stream=None) -> None:
        """Enqueue sha1chunk_index_lookup_device_async: digests a torch CUDA
        uint8 tensor of n x 20 bytes, ids one of n int32 (the uint32 positions)."""
        n = ids.numel() if n is None else n
        _check(lib().sha1chunk_index_lookup_device_async(self._ix, _addr(digests), n, _addr(ids), _stream_ptr(stream)),
               "sha1chunk_index_lookup_device_async")

    def match_batch(self, base, offsets, lengths, ids=None):
        """sha1chunk_match_batch: the position of every chunk's digest.  Host
        form (base bytes or a numpy array, offsets and lengths sequences)
        -> n uint32 positions; device form (torch CUDA tensors: base uint8,
        offsets int64, lengths int32, and ids int32 to receive the positions)
        -> ids."""
        if hasattr(base, "data_ptr"):
            if ids is None:
                raise ValueError("the device form needs an ids tensor")
            _check(lib().sha1chunk_match_batch(self._ix, _addr(base), _addr(offsets), _addr(lengths), offsets.numel(),
                                               _addr(ids), DEVICE), "sha1chunk_match_batch")
            return ids
        b = np.frombuffer(base, np.uint8) if isinstance(base, (bytes, bytearray)) else \
            np.ascontiguousarray(base).view(np.uint8).reshape(-1)
        if b.size == 0:
            b = np.zeros(1, np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        ln = np.ascontiguousarray(lengths, np.uint32)
        if off.shape != ln.shape:
            raise ValueError("offsets and lengths differ in length")
        out = np.full(off.size, NO_MATCH, np.uint32)
        _check(lib().sha1chunk_match_batch(self._ix, b.ctypes.data, off.ctypes.data, ln.ctypes.data, off.size,
                                           out.ctypes.data, HOST), "sha1chunk_match_batch")
        return out

    def match_fd(self, src, max_chunks: int | None = None) -> np.ndarray:
        """sha1chunk_match_fd: the position of every 512 KiB chunk of a file
        (a path, a binary file object on a real fd, or an fd) from its offset
        on -> uint32 positions, at most max_chunks of them."""
        if isinstance(src, (str, os.PathLike)):
            with open(src, "rb") as f:
                return self.match_fd(f, max_chunks)
        if isinstance(src, int):
            fd = src
        else:
            fd = src.fileno()
            os.lseek(fd, src.tell(), os.SEEK_SET)
        if max_chunks is None:
            size = os.fstat(fd).st_size - os.lseek(fd, 0, os.SEEK_CUR)
            max_chunks = max((size + CHUNK_LEN - 1) // CHUNK_LEN, 1)
        ids = np.full(max_chunks, NO_MATCH, np.uint32)
        total = C.c_size_t(0)
        n = _check(lib().sha1chunk_match_fd(self._ix, fd, ids.ctypes.data, max_chunks, C.byref(total)),
                   "sha1chunk_match_fd")
        return ids[:n]

    def close(self) -> None:
        if self._ix:
            lib().sha1chunk_index_destroy(self._ix)
            self._ix = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def has_chunks(data_path, chunk_list_path) -> list[tuple[int, bytes]]:
    """Which chunks of a chunk list a data file holds: (id in the list,
    digest) for every 512 KiB chunk of `data_path` whose digest is in
    `chunk_list_path` (a plain chunk file, or a master chunk file with its
    header line), in file order -- the lines of the peer's has-chunks file
    (the reference's tmp/B.haschunks: B.tar under ids 2 and 3 of
    C.masterchunks).  A digest listed under several ids gets the lowest."""
    from . import chunkfile
    entries = sorted(chunkfile.read_ids(chunk_list_path))
    with DigestIndex([bytes.fromhex(h) for _, h in entries]) as ix:
        pos = ix.match_fd(data_path)
    return [(entries[p][0], bytes.fromhex(entries[p][1])) for p in pos.tolist() if p != NO_MATCH]


def synth_fill_device(dst, first: int, count: int, chunk_len: int = CHUNK_LEN, seed: int = SEED,
                      stream=None) -> None:
    _check(lib().sha1chunk_synth_fill_async(dst.data_ptr(), first, count, chunk_len, seed,
                                            _stream_ptr(stream)), "sha1chunk_synth_fill_async")


def synth_fill_ragged_device(base, offsets, lengths, first: int, seed: int = SEED,
                             stream=None) -> None:
    _check(lib().sha1chunk_synth_fill_ragged_async(base.data_ptr(), offsets.data_ptr(),
                                                   lengths.data_ptr(), first, offsets.numel(),
                                                   seed, _stream_ptr(stream)),
           "sha1chunk_synth_fill_ragged_async")


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def mixed_lengths(n: int, seed: int = SEED) -> np.ndarray:
    """Chunk lengths of the synthetic mixed batch (BASELINE config 5, the
    received-chunk verify shape): chunk i draws an
    octave o in 0..7 and a mantissa m in 0..4095 from splitmix64 and is
    (4096 + m) << o bytes (4 KiB .. just under 1 MiB); every 7th chunk gets
    1..63 more bytes so its tail is not 64-byte aligned.  The golden digests
    of tests/golden/ were generated over these lengths by the reference."""
    i = np.arange(n, dtype=np.uint64)
    r = _splitmix64(np.uint64(seed + 1) ^ i)
    octave = (r & np.uint64(7)).astype(np.uint32)
    mant = ((r >> np.uint64(8)) & np.uint64(4095)).astype(np.uint32)
    ln = (np.uint32(4096) + mant) << octave
    tail = (_splitmix64(np.uint64(seed + 2) ^ i) % np.uint64(63)).astype(np.uint32) + 1
    return np.where(i % 7 == 6, ln + tail, ln).astype(np.uint32)


def ragged_layout(lengths: Iterable[int], align: int = 128) -> tuple[np.ndarray, int]:
    """Offsets packing chunks back to back at `align`-byte boundaries."""
    ln = np.asarray(list(lengths) if not isinstance(lengths, np.ndarray) else lengths, np.uint64)
    padded = (ln + (align - 1)) // align * align
    off = np.zeros(ln.size, np.uint64)
    if ln.size > 1:
        off[1:] = np.cumsum(padded)[:-1]
    total = int(padded.sum()) if ln.size else 0
    return off, total
