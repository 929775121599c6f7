"""The argument checks include/sha1chunk.h documents (SHA1CHUNK_EINVAL /
SHA1CHUNK_EALIGN), one table: every row is refused on the host -- no row
reaches a kernel with a bad pointer -- leaves the digest buffer it was given
unchanged, and leaves the library able to hash the next valid batch."""
import ctypes as C
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xAA
N_OK, LEN_OK = 65, 1001


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


class Ctx:
    """Buffers every row draws on: a valid 65 x 1001-byte batch on the device
    with its hashlib digests, and a digest buffer that starts as 0xAA."""

    def __init__(self, pkg, torch):
        self.pkg, self.torch, self.L = pkg, torch, pkg.lib()
        rng = np.random.default_rng(65)
        data = rng.integers(0, 256, N_OK * LEN_OK, dtype=np.uint8)
        raw = data.tobytes()
        self.want = np.frombuffer(b"".join(hashlib.sha1(raw[i * LEN_OK:(i + 1) * LEN_OK]).digest()
                                           for i in range(N_OK)), np.uint8).reshape(N_OK, 20)
        self.base = torch.from_numpy(data).cuda()
        self.off = torch.arange(N_OK, dtype=torch.int64, device="cuda") * LEN_OK
        self.len = torch.full((N_OK,), LEN_OK, dtype=torch.int32, device="cuda")
        self.dig = torch.full((N_OK * 20 + 64,), FILL, dtype=torch.uint8, device="cuda")
        self.mism = torch.full((N_OK + 64,), FILL, dtype=torch.uint8, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream
        # host side: the streaming trio's arguments
        self.state = np.array([0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0], np.uint32)
        self.block = np.zeros(64, np.uint8)
        self.hdig = np.full(20, FILL, np.uint8)
        torch.cuda.synchronize()

    def valid_call_is_right(self):
        out = self.torch.full((N_OK, 20), FILL, dtype=self.torch.uint8, device="cuda")
        self.pkg.hash_device(self.base, self.off, self.len, out, kernel="auto")
        assert np.array_equal(out.cpu().numpy(), self.want), "the valid call after a refused one is wrong"

    def buffers_untouched(self):
        self.torch.cuda.synchronize()
        assert (self.dig.cpu().numpy() == FILL).all(), "a refused call wrote to its digest buffer"
        assert (self.mism.cpu().numpy() == FILL).all(), "a refused call wrote to its mismatch buffer"
        assert (self.hdig == FILL).all(), "a refused call wrote to its host digest"
        assert self.state.tolist() == [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]


def _rows():
    """name -> (call(ctx) -> return value, expected code, substring of the
    error text).  An expected code of None: the call returns NULL."""
    E = {"OK": 0, "EINVAL": -1, "EALIGN": -5}
    rows = {}

    def ragged(x, base=True, off=True, ln=True, dig=0, n=1, kernel=0):
        return x.L.sha1chunk_hash_device_async(x.base.data_ptr() if base else None,
                                               x.off.data_ptr() if off else None,
                                               x.len.data_ptr() if ln else None, n,
                                               x.dig.data_ptr() + dig if dig is not None else None, x.st, kernel)

    def uniform(x, base=True, dig=0, n=1, kernel=0):
        return x.L.sha1chunk_hash_uniform_async(x.base.data_ptr() if base else None, LEN_OK, n,
                                                x.dig.data_ptr() + dig if dig is not None else None, x.st, kernel)

    for name, fn in (("hash_device_async", ragged), ("hash_uniform_async", uniform)):
        for kernel in (0, 1, 2, 3):
            rows[f"{name}: digests + 1, kernel {kernel}"] = (
                lambda x, fn=fn, k=kernel: fn(x, dig=1, n=N_OK, kernel=k), E["EALIGN"], "4-byte aligned")
        rows[f"{name}: digests + 2"] = (lambda x, fn=fn: fn(x, dig=2, n=1), E["EALIGN"], "4-byte aligned")
        rows[f"{name}: kernel id 7"] = (lambda x, fn=fn: fn(x, n=N_OK, kernel=7), E["EINVAL"], "unknown kernel id 7")
        rows[f"{name}: kernel id -1"] = (lambda x, fn=fn: fn(x, n=N_OK, kernel=-1), E["EINVAL"],
                                         "unknown kernel id -1")
        rows[f"{name}: null base"] = (lambda x, fn=fn: fn(x, base=False), E["EINVAL"], "null device pointer")
        rows[f"{name}: null digests"] = (lambda x, fn=fn: fn(x, dig=None), E["EINVAL"], "null device pointer")
        rows[f"{name}: n = 2^32"] = (lambda x, fn=fn: fn(x, n=2**32), E["EINVAL"], "n too large")
    rows["hash_device_async: null offsets"] = (lambda x: ragged(x, off=False), E["EINVAL"], "null device pointer")
    rows["hash_device_async: null lengths"] = (lambda x: ragged(x, ln=False), E["EINVAL"], "null device pointer")
    rows["hash_device_async: all null, n = 0"] = (
        lambda x: ragged(x, base=False, off=False, ln=False, dig=None, n=0), E["OK"], "")
    rows["hash_uniform_async: all null, n = 0"] = (lambda x: uniform(x, base=False, dig=None, n=0), E["OK"], "")

    def compare(x, dig=True, exp=True, mism=True, n=1):
        return x.L.sha1chunk_compare_device_async(x.dig.data_ptr() if dig else None,
                                                  x.base.data_ptr() if exp else None, n,
                                                  x.mism.data_ptr() if mism else None, x.st)

    rows["compare_device_async: null digests"] = (lambda x: compare(x, dig=False), E["EINVAL"], "null device pointer")
    rows["compare_device_async: null expected"] = (lambda x: compare(x, exp=False), E["EINVAL"],
                                                   "null device pointer")
    rows["compare_device_async: null mismatch"] = (lambda x: compare(x, mism=False), E["EINVAL"],
                                                   "null device pointer")
    rows["compare_device_async: n = 2^32"] = (lambda x: compare(x, n=2**32), E["EINVAL"], "n too large")
    rows["compare_device_async: all null, n = 0"] = (
        lambda x: compare(x, dig=False, exp=False, mism=False, n=0), E["OK"], "")

    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    rows["compress_blocks: nblocks = 2^26 + 1"] = (
        lambda x: x.L.sha1chunk_compress_blocks(x.state.ctypes.data_as(u32p), x.block.ctypes.data, 2**26 + 1),
        E["EINVAL"], "too many blocks")
    rows["compress_blocks: null blocks"] = (
        lambda x: x.L.sha1chunk_compress_blocks(x.state.ctypes.data_as(u32p), None, 1), E["EINVAL"], "null")
    rows["finish: tail_len = 64"] = (
        lambda x: x.L.sha1chunk_finish(x.state.ctypes.data_as(u32p), 0, x.block.ctypes.data, 64,
                                       x.hdig.ctypes.data_as(u8p)), E["EINVAL"], "bad argument")
    rows["finish: tail_len = 2^32 - 1"] = (
        lambda x: x.L.sha1chunk_finish(x.state.ctypes.data_as(u32p), 0, x.block.ctypes.data, 2**32 - 1,
                                       x.hdig.ctypes.data_as(u8p)), E["EINVAL"], "bad argument")
    rows["hash_stream_sized: null reader"] = (
        lambda x: x.L.sha1chunk_hash_stream_sized(x.pkg.sha1chunk.READER_FN(), None, x.pkg.sha1chunk.SINK_FN(),
                                                  None, 0), E["EINVAL"], "null reader")
    rows["hash_stream: null reader"] = (
        lambda x: x.L.sha1chunk_hash_stream(x.pkg.sha1chunk.READER_FN(), None, x.pkg.sha1chunk.SINK_FN(), None),
        E["EINVAL"], "null reader")
    for name, args in (("batch = 0", (0, 4096)), ("batch = 2^20 + 1", (2**20 + 1, 4096)),
                       ("max_chunk_len = 0", (16, 0))):
        rows[f"vq_create: {name}"] = (lambda x, a=args: x.L.sha1chunk_vq_create(*a), None,
                                      "batch 1..2^20 and max_chunk_len > 0")
    return rows


ROWS = _rows()


@pytest.fixture(scope="module")
def ctx(pkg, dev):
    c = Ctx(pkg, dev)
    c.valid_call_is_right()
    return c


@pytest.mark.parametrize("row", list(ROWS))
def test_refused_on_the_host(ctx, row):
    call, code, text = ROWS[row]
    # a marker in the thread's error text: a refusal must replace it
    assert ctx.L.sha1chunk_device_pci_bus_id(0, None, 0) == ctx.pkg.EINVAL
    assert ctx.L.sha1chunk_last_error() == b"null buffer"
    got = call(ctx)
    err = ctx.L.sha1chunk_last_error().decode()
    if code is None:
        assert got is None, f"{row}: returned a queue"
        assert text in err, err
    elif code == 0:
        assert got == 0, (got, err)
    else:
        assert got == code, (got, err)
        assert text in err, err
    ctx.buffers_untouched()
    ctx.valid_call_is_right()
