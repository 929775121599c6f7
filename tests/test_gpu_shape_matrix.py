"""GPU: every kernel shape with every batch feature, bit-exact against
hashlib.sha1.

The shapes are the lane and fused kernels and the split kernel's units 1, 4,
11 and 416 (the quad shape), each forced and each confirmed by its launch
counter (launch_stats.py; layout in csrc/sha1_kernels.h LaunchCounter), so a
case cannot pass by running some other kernel.  The features:

  order   A.order, the longest-first permutation, exists only behind
          kernel="auto" with more than 64 chunks.  SHA1CHUNK_FORCE_KERNEL (+
          SHA1CHUNK_SPLIT_UNIT) behind AUTO keeps the sort and makes the
          forced shape read the order: 65 chunks (a second, almost empty
          wave; the quad shape's last workgroup holds one chunk, its other
          quads fall back through the order), 130 (three groups: unit 11's
          last workgroup has an empty second pair) and 197, unsorted lengths
          with ties, chunks scattered in memory at byte misalignments 0..3;
          and 64 CUs' worth + 65 chunks, above the mixed kernel's threshold
          with the mixed kernel off.
  guards  the digest rows 4 bytes into a filled allocation, filled bytes
          after them: nothing outside n x 20 bytes changes.
  chains  the forced quad shape on one chunk of 512 KiB + 1 beside 15 short
          ones (thousands of masked-tail iterations), and AUTO's sorted quad
          path with one chunk of 4 MiB + 120, whose 16-bit sort key clamps.
"""
import hashlib

import numpy as np
import pytest

import launch_stats as LS

pytestmark = pytest.mark.gpu

SPLIT = "SHA1CHUNK_FORCE_KERNEL"
UNIT = "SHA1CHUNK_SPLIT_UNIT"
# shape -> (knobs behind kernel="auto", the counter of a ragged batch)
SHAPES = {
    "lane": ({SPLIT: "lane"}, "lane"),
    "fused": ({SPLIT: "fused"}, "fused"),
    "unit1": ({SPLIT: "split", UNIT: "1"}, "unit1"),
    "unit4": ({SPLIT: "split", UNIT: "4"}, "unit4"),
    "unit11": ({SPLIT: "split", UNIT: "11"}, "unit11_shared"),  # offsets and an order: the shared loads
    "unit416": ({SPLIT: "split", UNIT: "416"}, "quad"),
}
# the padding edges, and the quad consumer's block-count boundaries (test_gpu_quad_hoist.py BLOCKS)
EDGES = [0, 55, 56, 63, 64, 119, 120]
BLOCKS = [1, 2, 4, 5, 6, 7, 8, 9, 16, 17, 27]
BOUNDARY = EDGES + [64 * (t - 1) + 10 for t in BLOCKS]
FILL = 0xA5


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


@pytest.fixture(scope="module")
def cus(dev):
    return dev.cuda.get_device_properties(0).multi_processor_count


def lengths(n, seed, hi=5000):
    """n unsorted lengths with ties: every boundary length (twice where there
    is room), the rest random in 0..hi."""
    rng = np.random.default_rng(seed)
    fixed = [x for x in BOUNDARY * 2 if x <= hi][:max(0, n - 1)]
    lens = np.concatenate([np.array(fixed, np.int64), rng.integers(0, hi + 1, n - len(fixed))])
    return rng.permutation(lens).astype(np.uint32)


def layout(lens, mis, shuffled, seed):
    """Chunk i at a 16-byte boundary + mis with a gap after it; in memory in
    caller order, or in a random one (neighbours in the batch far apart)."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    step = (lens.astype(np.uint64) + np.uint64(15)) // np.uint64(16) * np.uint64(16) + np.uint64(16)
    perm = rng.permutation(n) if shuffled else np.arange(n)
    off = np.zeros(n, np.uint64)
    off[perm] = np.concatenate([[0], np.cumsum(step[perm])[:-1]]).astype(np.uint64)
    off += np.uint64(mis)
    host = rng.integers(0, 256, int((off + lens).max()) + 64, dtype=np.uint8)
    return host, off


def sha1_rows(host, off, lens):
    raw = host.tobytes()
    rows = np.frombuffer(b"".join(hashlib.sha1(raw[int(o):int(o) + int(m)]).digest() for o, m in zip(off, lens)),
                         np.uint8).reshape(len(lens), 20)
    rows.setflags(write=False)
    return rows


_cases = {}


def case(torch, key, make):
    """A batch on the device with hashlib's digests: built once per key,
    shared by the shapes, never written."""
    if key not in _cases:
        host, off, lens = make()
        _cases[key] = (torch.from_numpy(host).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
                       torch.from_numpy(lens.astype(np.int32)).cuda(), lens, sha1_rows(host, off, lens))
    return _cases[key]


def hash_guarded(pkg, torch, batch, kernel):
    """One call with the digests between guards; the counter delta."""
    d_host, d_off, d_len, lens, want = batch
    n = len(lens)
    raw = torch.full((4 + n * 20 + 64,), FILL, dtype=torch.uint8, device="cuda")
    dig = raw[4:4 + n * 20]
    assert dig.data_ptr() % 8 == 4
    torch.cuda.synchronize()
    before = LS.snapshot()
    pkg.hash_device(d_host, d_off, d_len, dig, kernel=kernel)
    torch.cuda.synchronize()
    launched = LS.delta(before)
    got = raw.cpu().numpy()
    bad = np.flatnonzero((got[4:4 + n * 20].reshape(n, 20) != want).any(axis=1))
    assert bad.size == 0, (f"{bad.size} of {n} digests differ from hashlib, first {bad[:8].tolist()}, "
                           f"lengths {lens[bad[:8]].tolist()}")
    assert (got[:4] == FILL).all() and (got[4 + n * 20:] == FILL).all(), "bytes around the digest rows written"
    return launched


# ---- order x shape ----------------------------------------------------------
@pytest.mark.parametrize("n", [65, 130, 197])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_order_with_every_shape(pkg, dev, monkeypatch, shape, n):
    torch = dev
    env, counter = SHAPES[shape]
    LS.clear_knobs(monkeypatch, **env)
    for mis in range(4):
        for shuffled in (False, True):
            def make():
                lens = lengths(n, 1000 + n)
                host, off = layout(lens, mis, shuffled, 8 * n + 2 * mis + shuffled)
                return host, off, lens
            launched = hash_guarded(pkg, torch, case(torch, ("order", n, mis, shuffled), make), "auto")
            assert launched == LS.expect(sort=1, **{counter: 1}), \
                f"{shape}, {n} chunks at +{mis}{' shuffled' if shuffled else ''}: launched {launched}"


@pytest.mark.parametrize("shape", list(SHAPES))
def test_order_above_the_cu_count(pkg, dev, cus, monkeypatch, shape):
    """More groups of 64 than CUs: AUTO alone would take the mixed kernel;
    with a forced kernel the shape itself gets the large sorted batch."""
    torch = dev
    env, counter = SHAPES[shape]
    LS.clear_knobs(monkeypatch, **env)
    n = 64 * cus + 65

    def make():
        lens = lengths(n, 77, hi=200)
        host, off = layout(lens, 1, True, 78)
        return host, off, lens
    launched = hash_guarded(pkg, torch, case(torch, ("big", n), make), "auto")
    assert launched == LS.expect(sort=1, **{counter: 1}), f"{shape}, {n} chunks: launched {launched}"


# ---- guards -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 65, 130])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_nothing_outside_the_digest_rows(pkg, dev, monkeypatch, shape, n):
    """Forced as kernel= (no order at any n) and behind AUTO (an order from
    65 chunks on): the bytes before and after the n x 20 digest bytes keep
    their fill."""
    torch = dev
    env, counter = SHAPES[shape]

    def make():
        lens = lengths(n, 2000 + n)
        host, off = layout(lens, n % 4, True, 2100 + n)
        return host, off, lens
    batch = case(torch, ("guard", n), make)
    LS.clear_knobs(monkeypatch, **env)
    launched = hash_guarded(pkg, torch, batch, "auto")
    assert launched == LS.expect(sort=int(n > 64), **{counter: 1}), f"{shape}, AUTO, {n} chunks: launched {launched}"
    LS.clear_knobs(monkeypatch, **{k: v for k, v in env.items() if k == UNIT})
    launched = hash_guarded(pkg, torch, batch, env[SPLIT])
    assert launched == LS.expect(**{counter: 1}), f"{shape}, kernel={env[SPLIT]}, {n} chunks: launched {launched}"


# ---- long chains in the quad shape -----------------------------------------
def test_quad_long_chain_in_one_workgroup(pkg, dev, monkeypatch):
    """16 chunks, one workgroup: one of 512 KiB + 1 (8193 blocks: 1024
    unrolled iterations and a masked tail of 1), the other 15 the shortest
    boundary lengths, which finish in the first iterations and stay masked."""
    torch = dev
    LS.clear_knobs(monkeypatch, **{UNIT: "416"})

    def make():
        lens = np.array(BOUNDARY[:15] + [(512 << 10) + 1], np.uint32)
        lens[[3, 15]] = lens[[15, 3]]  # the long chunk in the middle of the group
        host, off = layout(lens, 3, True, 512)
        return host, off, lens
    launched = hash_guarded(pkg, torch, case(torch, ("chain16",), make), "split")
    assert launched == LS.expect(quad=1), launched


def test_quad_sorted_with_a_clamped_key(pkg, dev, monkeypatch):
    """65 chunks through AUTO (sort, then the quad shape through the order):
    one chunk of 4 MiB + 120 (65539 blocks: its 16-bit sort key clamps) among
    64 short ones."""
    torch = dev
    LS.clear_knobs(monkeypatch)

    def make():
        lens = lengths(65, 4120)
        lens[41] = (4 << 20) + 120
        host, off = layout(lens, 1, True, 4121)
        return host, off, lens
    launched = hash_guarded(pkg, torch, case(torch, ("clamp65",), make), "auto")
    assert launched == LS.expect(sort=1, quad=1), launched
