"""Addresses across 2^32: every forced kernel, not only AUTO on the large
workloads, gets ragged offsets above 2^32 and a uniform layout whose
id * chunk_len passes 2^32.  One device buffer of 2^32 + 16 MiB serves both:
only a 16 MiB window centred on 2^32 (ragged, uploaded anew for each test)
or the synthetic fill (uniform) is ever written, so the tests cost an
allocation, not a 4 GiB upload."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T32 = 1 << 32
WIN = 16 << 20
LO = T32 - WIN // 2  # the window is [LO, LO + WIN)
ENV_KNOBS = ("SHA1CHUNK_MIXED_PLAN", "SHA1CHUNK_SPLIT_UNIT", "SHA1CHUNK_FORCE_KERNEL", "SHA1CHUNK_MIXED")


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


@pytest.fixture(scope="module")
def wide(dev):
    """An uninitialised device buffer of 2^32 + 16 MiB bytes."""
    torch = dev
    buf = torch.empty(T32 + WIN, dtype=torch.uint8, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def window_host():
    """16 MiB of random bytes: the contents of [2^32 - 8 MiB, 2^32 + 8 MiB)."""
    return np.frombuffer(np.random.default_rng(32).bytes(WIN), np.uint8).copy()


@pytest.fixture
def window(dev, wide, window_host):
    """The window uploaded into the device buffer, for every test that reads
    it (the uniform test's fill covers the same bytes, so no test relies on
    what another left there)."""
    wide[LO:LO + WIN].copy_(dev.from_numpy(window_host))
    dev.cuda.synchronize()
    return window_host


@pytest.fixture(scope="module")
def ragged(oracle, window_host):
    """130 byte-packed chunks of 0..70000 bytes; chunk 65 starts at 2^32 - 33
    and crosses the boundary, those before it lie below 2^32, those after it
    above.  Offsets are from the buffer's start; the oracle hashes the host
    copy of the window."""
    n = 130
    rng = np.random.default_rng(131)
    lens = rng.integers(0, 70001, n).astype(np.uint32)
    lens[[0, 3, 64, 65, 66, 129]] = [70000, 0, 55, 50000, 0, 119]
    off = np.zeros(n, np.uint64)
    off[0] = T32 - 33 - int(lens[:65].sum())
    off[1:] = off[0] + np.cumsum(lens[:-1], dtype=np.uint64)
    assert off[65] == T32 - 33 and off[0] >= LO and int(off[-1]) + int(lens[-1]) <= LO + WIN
    assert (off[:65] + lens[:65] <= T32).all() and (off[66:] >= T32).all()
    return off, lens, oracle.hash_batch(window_host, off - np.uint64(LO), lens)


def _hash_ragged(pkg, torch, wide, off, lens, kernel):
    n = lens.size
    dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    pkg.hash_device(wide, torch.from_numpy(off.astype(np.int64)).cuda(),
                    torch.from_numpy(lens.astype(np.int32)).cuda(), dig, kernel=kernel)
    torch.cuda.synchronize()
    return dig.cpu().numpy()


def _same(got, want, lens, off, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {lens.size} digests differ, first {bad[:8]}, "
                           f"lengths {lens[bad[:8]]}, offsets - 2^32 {off[bad[:8]].astype(np.int64) - T32}")


@pytest.mark.parametrize("kernel,unit", [("lane", None), ("fused", None), ("split", "1"), ("split", "4"),
                                         ("split", "11"), ("split", "416"), ("auto", None)])
def test_ragged_offsets_across_2_32(pkg, dev, wide, window, ragged, monkeypatch, kernel, unit):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    if unit:
        monkeypatch.setenv("SHA1CHUNK_SPLIT_UNIT", unit)
    off, lens, want = ragged
    _same(_hash_ragged(pkg, dev, wide, off, lens, kernel), want, lens, off, f"{kernel} {unit or ''}")


def test_mixed_kernel_across_2_32(pkg, dev, oracle, wide, window, monkeypatch):
    """More groups of 64 than CUs (AUTO's mixed kernel): 64 * (CUs + 1) - 5
    chunks of 0..700 bytes packed around 2^32, listed in another order than
    they lie in memory."""
    torch = dev
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    n = 64 * (torch.cuda.get_device_properties(0).multi_processor_count + 1) - 5
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 701, n).astype(np.uint32)
    lens[:8] = [0, 55, 56, 63, 64, 65, 119, 120]
    place = rng.permutation(n)  # memory position -> caller index
    lens[place[n // 2]] = 700  # the chunk in the middle of the layout crosses 2^32
    packed = lens[place]
    start = T32 - int(packed[:n // 2].sum()) - 17
    pos = np.zeros(n, np.uint64)
    pos[0] = start
    pos[1:] = start + np.cumsum(packed[:-1], dtype=np.uint64)
    assert pos[n // 2] == T32 - 17
    off = np.zeros(n, np.uint64)
    off[place] = pos
    assert off.min() >= LO and int((off + lens).max()) <= LO + WIN
    assert (off < T32).sum() > n // 3 and (off >= T32).sum() > n // 3
    want = oracle.hash_batch(window, off - np.uint64(LO), lens)
    _same(_hash_ragged(pkg, torch, wide, off, lens, "auto"), want, lens, off, "mixed")


def test_uniform_layout_across_2_32(pkg, dev, oracle, wide, monkeypatch):
    """4097 chunks of 1 MiB back to back: chunk 4096 starts at 2^32.  Chunks
    0, 4094, 4095 and 4096 against hashlib over the oracle's generator, the
    bytes of chunk 4096 against the generator, and all 4097 digests alike
    from every kernel."""
    torch = dev
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    L, n = 1 << 20, 4097
    pkg.synth_fill_device(wide, 0, n, L)
    probe = (0, 4094, 4095, 4096)
    src = {c: oracle.synth_chunk(c, L) for c in probe}
    assert np.array_equal(wide[4096 * L:4097 * L].cpu().numpy(), src[4096]), "bytes of chunk 4096"
    want = {c: hashlib.sha1(src[c].tobytes()).digest() for c in probe}
    first = None
    for kernel in ("lane", "fused", "split", "auto"):
        dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
        pkg.hash_uniform_device(wide, L, n, dig, kernel=kernel)
        torch.cuda.synchronize()
        got = dig.cpu().numpy()
        for c in probe:
            assert got[c].tobytes() == want[c], f"{kernel}: chunk {c}"
        if first is None:
            first = got
        else:
            bad = np.nonzero((got != first).any(axis=1))[0]
            assert bad.size == 0, f"{kernel} differs from lane at chunks {bad[:8]}"
