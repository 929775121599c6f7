"""The synthetic-corpus fills (sha1chunk_synth_fill_async and its ragged
variant) against the generator's definition: chunk c, 64-bit little-endian
word w = splitmix64(seed ^ (c << 24) ^ w), every operation modulo 2^64.  They
produce the input of bench.py and of every golden-digest test, so every byte
is compared -- with the CPU oracle's generator and with an independent numpy
statement of the formula -- and so is every byte the fill must not touch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0x5C
GUARD = 64
OTHER_SEED = 0xC0FFEE1234567
FIRSTS = (0, 17, 2**40 + 5)  # (2^40 + 5) << 24 does not fit 64 bits: the shift must wrap


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


def _np_chunk(c: int, length: int, seed: int) -> np.ndarray:
    """The header's formula in numpy, 64-bit wrap-around throughout."""
    mask = (1 << 64) - 1
    key = np.uint64((seed ^ ((c << 24) & mask)) & mask)
    w = np.arange((length + 7) // 8, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (key ^ w) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z.astype("<u8").view(np.uint8)[:length]


def _ref_chunk(oracle, c: int, length: int, seed: int) -> np.ndarray:
    """Chunk c from the oracle's generator; the two references must agree."""
    a = oracle.synth_chunk(c & ((1 << 64) - 1), length, seed)
    assert np.array_equal(a, _np_chunk(c, length, seed)), (c, length, seed)
    return a


def _filled(torch, nbytes: int):
    """An 8-byte aligned device buffer of nbytes + guard, all FILL."""
    t = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 8 == 0
    return t


@pytest.mark.parametrize("chunk_len,count", [(8, 1), (24, 3), (4096, 257), (2056, 5)])
def test_uniform_fill(pkg, dev, oracle, chunk_len, count):
    """count chunks of chunk_len bytes back to back, for three first-chunk
    indices (one whose shift overflows) and two seeds: every byte equals the
    reference, the 64 bytes behind the last chunk keep their fill."""
    torch = dev
    for first in FIRSTS:
        for seed in (pkg.SEED, OTHER_SEED):
            buf = _filled(torch, chunk_len * count)
            pkg.synth_fill_device(buf, first, count, chunk_len, seed)
            got = buf.cpu().numpy()
            want = np.concatenate([_ref_chunk(oracle, first + c, chunk_len, seed) for c in range(count)])
            bad = np.nonzero(got[:want.size] != want)[0]
            assert bad.size == 0, f"first={first} seed={seed:#x}: {bad.size} bytes differ, first at {bad[:4]}"
            assert (got[want.size:] == FILL).all(), f"first={first} seed={seed:#x}: guard written"


@pytest.mark.parametrize("chunk_len", [0, 1, 7, 13, 4099])
def test_single_chunk_any_length(pkg, dev, oracle, chunk_len):
    """count == 1 takes any chunk_len; a length that is no multiple of 8 ends
    in a partial word written byte by byte.  Nothing behind chunk_len is
    written."""
    torch = dev
    for first in FIRSTS:
        for seed in (pkg.SEED, OTHER_SEED):
            buf = _filled(torch, chunk_len)
            pkg.synth_fill_device(buf, first, 1, chunk_len, seed)
            got = buf.cpu().numpy()
            assert np.array_equal(got[:chunk_len], _ref_chunk(oracle, first, chunk_len, seed)), (first, seed)
            assert (got[chunk_len:] == FILL).all(), f"first={first}: bytes behind the chunk written"


def test_ragged_fill(pkg, dev, oracle):
    """130 chunks of 0..4097 bytes at 8-byte aligned offsets with gaps of 8 to
    39 bytes between them, laid out in another order than their indices:
    chunk i is oracle.synth_chunk(first + i, len[i]) and every byte between
    and behind the chunks keeps its fill."""
    torch = dev
    n = 130
    rng = np.random.default_rng(130)
    lens = rng.integers(0, 600, n).astype(np.uint32)
    lens[:7] = [0, 1, 7, 8, 9, 63, 4097]
    place = rng.permutation(n)  # layout position -> chunk index
    off = np.zeros(n, np.uint64)
    cur = 8
    for i in place:
        off[i] = cur
        end = cur + int(lens[i])
        cur = (end + 8 + 7) // 8 * 8 + 8 * int(rng.integers(0, 4))
        assert 8 <= cur - end <= 39
    assert (off % 8 == 0).all() and not np.array_equal(np.argsort(off), np.arange(n))
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_len = torch.from_numpy(lens.astype(np.int32)).cuda()
    for first, seed in ((0, pkg.SEED), (2**40 + 5, OTHER_SEED)):
        buf = _filled(torch, cur)
        pkg.synth_fill_ragged_device(buf, d_off, d_len, first, seed)
        got = buf.cpu().numpy()
        want = np.full(cur + GUARD, FILL, np.uint8)
        for i in range(n):
            want[int(off[i]):int(off[i]) + int(lens[i])] = _ref_chunk(oracle, first + i, int(lens[i]), seed)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"first={first}: {bad.size} bytes differ, first at {bad[:8]}"


def _refused(pkg, torch, buf, rc, code, text):
    assert rc == code, (rc, pkg.lib().sha1chunk_last_error())
    assert text in pkg.lib().sha1chunk_last_error().decode(), pkg.lib().sha1chunk_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all(), "a refused fill wrote to the buffer"


def test_refused_fills_write_nothing(pkg, dev):
    """Several chunks of a length that is no multiple of 8 and a destination
    off 8-byte alignment are SHA1CHUNK_EALIGN, a null destination with
    count > 0 SHA1CHUNK_EINVAL; the buffer is unchanged after each."""
    torch = dev
    L = pkg.lib()
    st = torch.cuda.current_stream().cuda_stream
    buf = _filled(torch, 256)
    p = buf.data_ptr()
    for chunk_len in (7, 12, 100):
        _refused(pkg, torch, buf, L.sha1chunk_synth_fill_async(p, 0, 2, chunk_len, pkg.SEED, st),
                 pkg.EALIGN, "8-byte")
    for shift in (1, 4):
        for count, chunk_len in ((1, 8), (2, 16), (1, 5)):
            _refused(pkg, torch, buf, L.sha1chunk_synth_fill_async(p + shift, 0, count, chunk_len, pkg.SEED, st),
                     pkg.EALIGN, "8-byte")
    _refused(pkg, torch, buf, L.sha1chunk_synth_fill_async(None, 0, 1, 8, pkg.SEED, st), pkg.EINVAL, "null")
    d_off = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_len = torch.full((1,), 8, dtype=torch.int32, device="cuda")
    for args in ((None, d_off.data_ptr(), d_len.data_ptr()), (p, None, d_len.data_ptr()),
                 (p, d_off.data_ptr(), None)):
        _refused(pkg, torch, buf, L.sha1chunk_synth_fill_ragged_async(*args, 0, 1, pkg.SEED, st),
                 pkg.EINVAL, "null")
    # a count of 0 is no error, with or without pointers
    assert L.sha1chunk_synth_fill_async(None, 0, 0, 8, pkg.SEED, st) == pkg.OK
    assert L.sha1chunk_synth_fill_ragged_async(None, None, None, 0, 0, pkg.SEED, st) == pkg.OK
    # and the next valid fill is right
    pkg.synth_fill_device(buf, 3, 2, 16)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:32], np.concatenate([_np_chunk(3, 16, pkg.SEED), _np_chunk(4, 16, pkg.SEED)]))
    assert (got[32:] == FILL).all()


def test_count_beyond_one_launch_is_refused(pkg, dev):
    """One workgroup per chunk: a count the launch cannot express is
    SHA1CHUNK_EINVAL before any launch, not a fill of count mod 2^32 chunks.
    count = 2^32 + 1 with chunk_len 8 on a 64-byte buffer: truncated, it
    would be one 8-byte chunk, so the call stays inside the buffer whether or
    not it is refused."""
    torch = dev
    L = pkg.lib()
    st = torch.cuda.current_stream().cuda_stream
    count = 2**32 + 1
    buf = torch.full((64,), FILL, dtype=torch.uint8, device="cuda")
    _refused(pkg, torch, buf, L.sha1chunk_synth_fill_async(buf.data_ptr(), 0, count, 8, pkg.SEED, st),
             pkg.EINVAL, "at most")
    d_off = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_len = torch.full((1,), 8, dtype=torch.int32, device="cuda")
    _refused(pkg, torch, buf,
             L.sha1chunk_synth_fill_ragged_async(buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), 0, count,
                                                 pkg.SEED, st), pkg.EINVAL, "at most")


def test_largest_count_of_one_launch(pkg, dev):
    """One 256-thread workgroup per chunk and fewer than 2^32 work-items per
    launch: 2^24 - 1 chunks is the most one call fills, 2^24 is refused.  The
    buffer holds 2^24 chunks of 8 bytes, so neither call can leave it.  Chunk
    c is the single word splitmix64(seed ^ (c << 24))."""
    torch = dev
    L = pkg.lib()
    st = torch.cuda.current_stream().cuda_stream
    top = 1 << 24
    buf = _filled(torch, 8 * top)
    rc = L.sha1chunk_synth_fill_async(buf.data_ptr(), 0, top, 8, pkg.SEED, st)
    assert rc == pkg.EINVAL and "at most" in L.sha1chunk_last_error().decode(), (rc, L.sha1chunk_last_error())
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()), "a refused fill wrote to the buffer"
    pkg.synth_fill_device(buf, 5, top - 1, 8)
    got = buf.cpu().numpy()
    c = np.arange(5, 5 + top - 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (np.uint64(pkg.SEED) ^ (c << np.uint64(24))) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    bad = np.nonzero(got[:8 * (top - 1)].view("<u8") != z)[0]
    assert bad.size == 0, f"{bad.size} chunks differ, first {bad[:4]}"
    assert (got[8 * (top - 1):] == FILL).all(), "bytes behind the last chunk written"
