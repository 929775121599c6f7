"""The C ABI around the kernels, device-memory side: sha1chunk_hash_batch and
sha1chunk_verify_batch with SHA1CHUNK_DEVICE (every buffer a device pointer,
slot 0's scratch and stream inside the library) and the compare kernel.
Expected digests are hashlib's; expected flags are stated by the test."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

pytestmark = pytest.mark.gpu

EDGE_LENS = [120, 0, 55, 56, 63, 64, 65, 119]  # both sides of the one-/two-block padding edge
GUARD = 64
FILL = 0xAA


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


def _cus(torch) -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ragged_case(n: int, seed: int, first_off: int = 37, max_len: int = 700):
    """n chunks of 0..max_len bytes (the padding-edge lengths first), byte-packed
    from a non-zero first offset: (bytes, offsets, lengths, hashlib digests)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n).astype(np.uint32)
    k = min(n, len(EDGE_LENS))
    lens[:k] = EDGE_LENS[:k]
    off = np.zeros(n, np.uint64)
    off[0] = first_off
    if n > 1:
        off[1:] = first_off + np.cumsum(lens[:-1], dtype=np.uint64)
    total = int(off[-1]) + int(lens[-1])
    data = rng.integers(0, 256, total + 16, dtype=np.uint8)
    raw = data.tobytes()
    want = np.frombuffer(b"".join(hashlib.sha1(raw[int(o):int(o) + int(l)]).digest()
                                  for o, l in zip(off, lens)), np.uint8).reshape(n, 20)
    return data, off, lens, want


def _to_dev(torch, data, off, lens):
    return (torch.from_numpy(data).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
            torch.from_numpy(lens.astype(np.int32)).cuda())


# ------------------------------------------------ hash_batch, DEVICE ------
HASH_BATCH_SIZES = {"1": 1, "64": 64, "65": 65, "200": 200, "mixed": None}  # mixed: 64 * (CUs + 1) - 7


@pytest.mark.parametrize("size", list(HASH_BATCH_SIZES))
def test_hash_batch_device(pkg, dev, size):
    """sha1chunk_hash_batch(SHA1CHUNK_DEVICE) on ragged byte-packed chunks: one
    chunk, one wave, one wave + 1, several waves, and more groups of 64 than
    CUs (AUTO's mixed kernel).  The digest buffer starts 4 bytes into an
    allocation (4-byte aligned, no more); the bytes around it keep their
    fill.  The call is synchronous: the result is read back on PyTorch's
    stream with no synchronisation of the library's own."""
    torch = dev
    n = HASH_BATCH_SIZES[size] or 64 * (_cus(torch) + 1) - 7
    data, off, lens, want = _ragged_case(n, 100 + list(HASH_BATCH_SIZES).index(size))
    d_base, d_off, d_len = _to_dev(torch, data, off, lens)
    raw = torch.full((4 + n * 20 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    dig = raw[4:4 + n * 20]
    assert dig.data_ptr() % 8 == 4
    torch.cuda.synchronize()  # the fill above; nothing after the call
    pkg.hash_batch_device(d_base, d_off, d_len, dig)
    got = raw.cpu().numpy()
    bad = np.nonzero((got[4:4 + n * 20].reshape(n, 20) != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {n} digests differ from hashlib, first {bad[:8]}, lens {lens[bad[:8]]}"
    assert (got[:4] == FILL).all() and (got[4 + n * 20:] == FILL).all(), "bytes around the digests written"


# ---------------------------------------------- verify_batch, DEVICE ------
CORRUPT_BYTES = (0, 3, 4, 16, 19)  # every 32-bit word of a digest, both ends


def _corrupt_at(n: int):
    """Chunk -> (digest byte, bit): the first and last chunk, both sides of
    the compare kernel's 256-thread block where n reaches it, one between."""
    idx = sorted({0, min(7, n - 1), min(255, n // 2), min(256, n - 2), n - 1})
    assert len(idx) == len(CORRUPT_BYTES)
    return {i: (CORRUPT_BYTES[k], (3 * k + 1) % 8) for k, i in enumerate(idx)}


def _verify_device(pkg, torch, n: int, seed: int, max_len: int = 700) -> np.ndarray:
    """One DEVICE verify of n ragged chunks against hashlib digests with
    _corrupt_at(n) flipped; returns the mismatch buffer with its guard."""
    data, off, lens, want = _ragged_case(n, seed, max_len=max_len)
    exp = want.copy()
    for i, (byte, bit) in _corrupt_at(n).items():
        exp[i, byte] ^= 1 << bit
    d_base, d_off, d_len = _to_dev(torch, data, off, lens)
    d_exp = torch.from_numpy(exp).cuda()
    mism = torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pkg.verify_batch_device(d_base, d_off, d_len, d_exp, mism, n=n)
    return mism.cpu().numpy()


def _check_verify(mism: np.ndarray, n: int):
    flagged = np.nonzero(mism[:n] == 1)[0].tolist()
    assert flagged == sorted(_corrupt_at(n)), f"n={n}: flagged {flagged}"
    clean = np.setdiff1d(np.arange(n), flagged)
    assert (mism[clean] == 0).all(), f"n={n}: entries neither 0 nor 1: {np.unique(mism[clean])}"
    assert (mism[n:] == FILL).all(), f"n={n}: bytes past n written"


GROW = (1 << 20) // 20 + 65  # digests beyond the 1 MiB the library's scratch buffers start with


def _verify_sizes(torch):
    """Small; more groups of 64 than CUs (the mixed kernel); small again; a
    batch whose digests outgrow slot 0's scratch (the buffer is freed and
    allocated anew); small once more."""
    return [(70, 7, 700), (64 * (_cus(torch) + 1), 8, 700), (70, 7, 700), (GROW, 9, 150), (70, 7, 700)]


def _verify_scenario(pkg, torch):
    """The verifies of _verify_sizes in one process.  Returns [[n, flagged
    indices]]."""
    out = []
    for n, seed, max_len in _verify_sizes(torch):
        mism = _verify_device(pkg, torch, n, seed, max_len)
        _check_verify(mism, n)
        out.append([n, np.nonzero(mism[:n])[0].tolist()])
    return out


def test_verify_batch_device(pkg, dev):
    """sha1chunk_verify_batch(SHA1CHUNK_DEVICE): `expected` and `mismatch` in
    device memory, one bit flipped in five expected digests (bytes 0, 3, 4,
    16, 19).  Exactly those entries are 1, every other is 0 (the buffer
    starts as 0xAA), the 64 bytes behind n stay 0xAA; n = 70, then n =
    64 * (CUs + 1), then the first batch again, then a batch that makes the
    library's digest scratch grow, and the first batch once more."""
    res = _verify_scenario(pkg, dev)
    assert res[0] == res[2] == res[4]


_CHILD = r"""
import importlib, json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import torch
m = importlib.import_module("congestion-control-with-bittorren_amd")
import test_gpu_abi_device as T
torch.cuda.set_device(0)
print("RESULT " + json.dumps(T._verify_scenario(m, torch)))
"""


def test_verify_batch_device_first_call_of_a_process(pkg, dev):
    """The same verifies as the first library calls of a fresh process: slot
    0's scratch and stream have had no earlier use (no set_device, no
    device_count, no hash before it)."""
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, TESTS], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, r.stdout + r.stderr
    res = json.loads(line[0][7:])
    assert res == [[n, sorted(_corrupt_at(n))] for n, _, _ in _verify_sizes(dev)]


# ------------------------------------------------------ compare kernel ----
def _compare_case(n: int, corrupt: bool):
    rng = np.random.default_rng(1000 + n)
    dig = rng.integers(0, 256, (max(n, 1), 20), dtype=np.uint8)[:n]
    exp = dig.copy()
    flagged = [i for i in range(n) if i % 3 == 0] if corrupt else []
    for i in flagged:
        exp[i, i % 20] ^= 1 << (i % 8)
    return dig, exp, flagged


_COMPARE_CASES = [(n, c, False) for n in (0, 1, 255, 256, 257, 1000) for c in (True, False)] + \
    [(257, True, True), (1000, True, True)]


@pytest.mark.parametrize("n,corrupt,odd", _COMPARE_CASES,
                         ids=[f"{n}-{'corrupt' if c else 'clean'}{'-odd-address' if o else ''}"
                              for n, c, o in _COMPARE_CASES])
def test_compare_kernel(pkg, dev, n, corrupt, odd):
    """sha1chunk_compare_device_async: chunk i (i % 3 == 0) differs from its
    expected digest in one bit, at byte i % 20, bit i % 8 -- over 1000 chunks
    every byte position and bit.  Exactly those entries become 1, all others
    0 (the buffer starts as 0xAA), the 64 bytes behind n and, for n = 0, the
    whole buffer keep 0xAA.  `odd-address`: both digest arrays start at byte
    1 of their allocation (the kernel is byte-wise; the header promises no
    alignment)."""
    torch = dev
    dig, exp, flagged = _compare_case(n, corrupt)
    shift = 1 if odd else 0
    d_dig = torch.zeros(n * 20 + 1 + shift, dtype=torch.uint8, device="cuda")[shift:shift + n * 20]
    d_exp = torch.zeros(n * 20 + 1 + shift, dtype=torch.uint8, device="cuda")[shift:shift + n * 20]
    if n:
        d_dig.copy_(torch.from_numpy(dig.reshape(-1)))
        d_exp.copy_(torch.from_numpy(exp.reshape(-1)))
        assert d_dig.data_ptr() % 2 == shift and d_exp.data_ptr() % 2 == shift
    mism = torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    rc = pkg.lib().sha1chunk_compare_device_async(d_dig.data_ptr(), d_exp.data_ptr(), n, mism.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream)
    assert rc == pkg.OK, pkg.lib().sha1chunk_last_error()
    got = mism.cpu().numpy()
    assert np.nonzero(got[:n] == 1)[0].tolist() == flagged
    rest = np.setdiff1d(np.arange(n), flagged)
    assert (got[rest] == 0).all(), f"entries neither 0 nor 1: {np.unique(got[rest])}"
    assert (got[n:] == FILL).all(), "bytes past n written"
