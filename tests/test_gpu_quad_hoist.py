"""GPU: the quad split consumer after its rounds were re-laid (csrc/sha1_split.hpp
kVQuad: the read burst, 80 rounds with no wait between them, the burst's
lgkmcnt(0) after round 79, then the feed-forward; the first W+K set and the
initial state waited for in front of the loop), forced
(SHA1CHUNK_SPLIT_UNIT=416) and through AUTO,
bit-exact against hashlib.sha1; that both calls ran the quad shape is read
from the backend's launch counters (launch_stats.py).

The unit stayed at U = 4 blocks (the 8-block unit lost its gate), so the
boundaries are: R = 4, the round the old in-block wait stood at (and 5, the
most rounds whose adds could be moved in front of the burst), the unit (4
blocks), the consumer's unrolled iteration (2U = 8 blocks) and its masked
tail.  Lengths are chosen by their SHA-1 block count T (data blocks plus
padding), chunk counts by workgroup (16 chunks each).  Shapes are tiny: the
largest chunk is 27 blocks."""
import hashlib

import numpy as np
import pytest

import launch_stats as LS

pytestmark = pytest.mark.gpu

QUAD = "416"
U = 4
# T blocks <- length 64 (T - 1) + 10: 1, 2, R, R + 1 (R = 4 and 5), 2U - 1, 2U, 2U + 1, 4U, 4U + 1, 6U + 3
BLOCKS = [1, 2, 4, 5, 6, 2 * U - 1, 2 * U, 2 * U + 1, 4 * U, 4 * U + 1, 6 * U + 3]
# the padding edges: 55 | 56 (one block | two), 119 | 120 (two | three), and the empty message
EDGES = [0, 55, 56, 119, 120]
COUNTS = [1, 15, 16, 17, 33]
MODES = {"forced": ("split", {"SHA1CHUNK_SPLIT_UNIT": QUAD}), "auto": ("auto", {})}
KNOBS = ("SHA1CHUNK_SPLIT_UNIT", "SHA1CHUNK_FORCE_KERNEL", "SHA1CHUNK_MIXED", "SHA1CHUNK_MIXED_PLAN")


def blocks_of(length):
    return length // 64 + (1 if length % 64 < 56 else 2)


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def placed(rng, lens, mis):
    """Chunk i at a 16-byte boundary + mis, a gap after each."""
    step = (lens.astype(np.uint64) + 15) // 16 * 16 + 16
    off = np.zeros(len(lens), np.uint64)
    off[1:] = np.cumsum(step)[:-1]
    off += np.uint64(mis)
    host = rng.integers(0, 256, int(off[-1] + lens[-1]) + 64, dtype=np.uint8)
    return host, off


def check(pkg, torch, monkeypatch, host, off, lens, what):
    n = len(lens)
    want = np.array([np.frombuffer(hashlib.sha1(host[int(o):int(o) + int(m)].tobytes()).digest(), np.uint8)
                     for o, m in zip(off, lens)], np.uint8).reshape(n, 20)
    d_host = torch.from_numpy(host).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_len = torch.from_numpy(lens.astype(np.int32)).cuda()
    for mode, (kernel, env) in MODES.items():
        set_env(monkeypatch, env)
        dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
        before = LS.snapshot()
        pkg.hash_device(d_host, d_off, d_len, dig, kernel=kernel)
        torch.cuda.synchronize()
        launched = LS.delta(before)
        bad = np.flatnonzero((dig.cpu().numpy() != want).any(axis=1))
        assert bad.size == 0, f"{what}, {mode}: {bad.size} of {n} digests differ, first {bad[:8].tolist()}"
        # both arms ran the quad shape and no other hash kernel (n <= 64 here: no sort either)
        assert launched == LS.expect(quad=1), f"{what}, {mode}: launched {launched}"


def test_block_counts_are_the_boundaries():
    """The lengths used below have the block counts they are meant to have."""
    assert [blocks_of(64 * (t - 1) + 10) for t in BLOCKS] == BLOCKS
    assert [blocks_of(x) for x in EDGES] == [1, 1, 2, 2, 3]


@pytest.mark.parametrize("n", COUNTS)
def test_uniform_block_counts(pkg, dev, monkeypatch, n):
    """Every chunk of the batch T blocks long: whole unrolled iterations
    (T a multiple of 2U), the masked tail alone (T < 2U), and both."""
    rng = np.random.default_rng(1000 + n)
    for length in [64 * (t - 1) + 10 for t in BLOCKS] + EDGES:
        lens = np.full(n, length, np.uint32)
        host, off = placed(rng, lens, n % 4)
        check(pkg, dev, monkeypatch, host, off, lens, f"{n} x {length} B ({blocks_of(length)} blocks)")


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_one_group_sixteen_lengths(pkg, dev, monkeypatch, mis):
    """One workgroup whose 16 quads end at 16 different blocks: some inside
    the first unrolled iteration (T <= 2U), some in a later one, some in the
    masked tail, in ascending and in a shuffled lane order."""
    rng = np.random.default_rng(50 + mis)
    lens = np.array([64 * (t - 1) + 10 for t in BLOCKS] + EDGES, np.uint32)
    assert len(lens) == 16
    for order in (lens, rng.permutation(lens)):
        host, off = placed(rng, order, mis)
        check(pkg, dev, monkeypatch, host, off, order, f"16 lengths at +{mis}")


@pytest.mark.parametrize("mode", list(MODES))
def test_initial_state_across_two_units(pkg, dev, monkeypatch, mode):
    """Batched SHA1Update from non-IV states (update mode: whole blocks, raw
    state out; the state is loaded from memory and waited for in front of
    the loop): second pieces of 2U - 1, 2U and 2U + 1 whole blocks and their
    neighbours, 17 contexts (two workgroups)."""
    torch = dev
    set_env(monkeypatch, MODES[mode][1])
    rng = np.random.default_rng(23)
    n = 17
    whole = [2 * U - 1, 2 * U, 2 * U + 1, 1, 4 * U, 4 * U + 1, 2 * U - 2]
    first = [rng.integers(0, 256, 64 * (1 + i % 3) + (i % 5), dtype=np.uint8) for i in range(n)]
    second = [rng.integers(0, 256, 64 * whole[i % len(whole)] + (7 * i) % 64, dtype=np.uint8) for i in range(n)]
    ctx = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    pkg.init_contexts_device(ctx, n=n, n_contexts=n)
    keep = []  # the pieces' device buffers, until the work on them is done
    for pieces in (first, second):
        lens = np.array([len(p) for p in pieces], np.uint32)
        off = np.zeros(n, np.uint64)
        off[1:] = np.cumsum(lens.astype(np.uint64) + 5)[:-1]
        host = np.zeros(int(off[-1] + lens[-1]) + 64, np.uint8)
        for p, o in zip(pieces, off):
            host[int(o):int(o) + len(p)] = p
        keep.append((torch.from_numpy(host).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
                     torch.from_numpy(lens.astype(np.int32)).cuda()))
        pkg.update_contexts_device(ctx, *keep[-1], n=n, n_contexts=n)
    dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    pkg.final_contexts_device(ctx, dig, n=n, n_contexts=n)
    torch.cuda.synchronize()
    got = dig.cpu().numpy()
    for i in range(n):
        want = hashlib.sha1(first[i].tobytes() + second[i].tobytes()).digest()
        assert got[i].tobytes() == want, f"context {i} ({mode})"
