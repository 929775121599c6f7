"""GPU: the quad shape of the split kernel (csrc/sha1_split.hpp kVQuad: four
lanes per chunk, 16 chunks per workgroup, SHA1CHUNK_SPLIT_UNIT=416), forced
and through AUTO (which picks it up to 16 chunks per CU), bit-exact against
hashlib.sha1: partial and whole groups, every padding case, several consumer
iterations plus a masked tail, lanes of one group ending at different blocks,
byte-misaligned chunks, the dispatch rule at its own chunk count and its
neighbour, and a non-IV initial state (batched SHA1Update).  That the forced
and the AUTO call ran the quad shape (and the neighbour count the 4-block-unit
shape) is read from the backend's launch counters (launch_stats.py)."""
import hashlib

import numpy as np
import pytest

import launch_stats as LS

pytestmark = pytest.mark.gpu

QUAD = "416"
COUNTS = [1, 3, 15, 16, 17, 33]
# 64*16*3 + 5: 49 blocks = three consumer iterations of 2U = 8 blocks and a masked tail
LENGTHS = [0, 1, 55, 56, 63, 64, 119, 120, 511, 512, 513, 1024 + 3, 64 * 16 * 3 + 5]
RAGGED = [0, 1, 55, 56, 63, 64, 119, 200, 511, 777, 1024, 1500, 2047, 2500, 3000, 3071]
# the shape forced, and AUTO's own choice
MODES = {"forced": ("split", {"SHA1CHUNK_SPLIT_UNIT": QUAD}), "auto": ("auto", {})}
KNOBS = ("SHA1CHUNK_SPLIT_UNIT", "SHA1CHUNK_FORCE_KERNEL", "SHA1CHUNK_MIXED", "SHA1CHUNK_MIXED_PLAN")


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


def sha1_rows(host, off, lens):
    return np.array([np.frombuffer(hashlib.sha1(host[int(o):int(o) + int(n)].tobytes()).digest(), np.uint8)
                     for o, n in zip(off, lens)], np.uint8).reshape(len(lens), 20)


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check(pkg, torch, monkeypatch, host, off, lens, what, uniform=None):
    """Hash the batch forced and through AUTO; uniform = L: back to back
    through the uniform entry point (no offset array)."""
    n = len(lens)
    want = sha1_rows(host, off, lens)
    d_host = torch.from_numpy(host).cuda()
    for mode, (kernel, env) in MODES.items():
        set_env(monkeypatch, env)
        dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
        before = LS.snapshot()
        if uniform is not None:
            pkg.hash_uniform_device(d_host, uniform, n, dig, kernel=kernel)
        else:
            d_off = torch.from_numpy(off.astype(np.int64)).cuda()
            d_len = torch.from_numpy(lens.astype(np.int32)).cuda()
            pkg.hash_device(d_host, d_off, d_len, dig, kernel=kernel)
        torch.cuda.synchronize()
        launched = LS.delta(before)
        bad = np.flatnonzero((dig.cpu().numpy() != want).any(axis=1))
        assert bad.size == 0, f"{what}, {mode}: {bad.size} of {n} digests differ, first {bad[:8].tolist()}"
        # both arms ran the quad shape and no other hash kernel (n <= 64 here: no sort either)
        assert launched == LS.expect(quad=1), f"{what}, {mode}: launched {launched}"


def placed(rng, lens, mis):
    """Chunk i at a 16-byte boundary + mis, a gap after each."""
    step = (lens.astype(np.uint64) + 15) // 16 * 16 + 16
    off = np.zeros(len(lens), np.uint64)
    off[1:] = np.cumsum(step)[:-1]
    off += np.uint64(mis)
    host = rng.integers(0, 256, int(off[-1] + lens[-1]) + 64, dtype=np.uint8)
    return host, off


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
@pytest.mark.parametrize("n", COUNTS)
def test_uniform_lengths(pkg, dev, monkeypatch, n, mis):
    rng = np.random.default_rng(416 * n + mis)
    for L in LENGTHS:
        lens = np.full(n, L, np.uint32)
        if mis == 0:  # back to back, no offset array (odd lengths misalign the chunks by themselves)
            host = rng.integers(0, 256, n * L + 64, dtype=np.uint8)
            check(pkg, dev, monkeypatch, host, np.arange(n, dtype=np.uint64) * np.uint64(L), lens,
                  f"{n} x {L} B uniform", uniform=L)
        host, off = placed(rng, lens, mis)
        check(pkg, dev, monkeypatch, host, off, lens, f"{n} x {L} B at +{mis}")


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_ragged_group(pkg, dev, monkeypatch, mis):
    """One group of 16 chunks of 16 different lengths: its quads end at
    different blocks (the masked commit), in two lane orders."""
    rng = np.random.default_rng(7 + mis)
    for lens in (np.array(RAGGED, np.uint32), rng.permutation(np.array(RAGGED, np.uint32))):
        host, off = placed(rng, lens, mis)
        check(pkg, dev, monkeypatch, host, off, lens, f"ragged group at +{mis}")


@pytest.mark.parametrize("n", [4096, 4097])
def test_dispatch_boundary(pkg, dev, monkeypatch, n):
    """AUTO at the workload's chunk count (16 chunks per CU on 256 CUs: the
    quad shape) and one chunk beyond it (the 4-block-unit shape)."""
    torch = dev
    L = 256
    rng = np.random.default_rng(n)
    host = rng.integers(0, 256, n * L, dtype=np.uint8)
    lens = np.full(n, L, np.uint32)
    want = sha1_rows(host, np.arange(n, dtype=np.uint64) * np.uint64(L), lens)
    set_env(monkeypatch, {})
    dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    d_host = torch.from_numpy(host).cuda()
    before = LS.snapshot()
    pkg.hash_uniform_device(d_host, L, n, dig, kernel="auto")
    torch.cuda.synchronize()
    launched = LS.delta(before)
    bad = np.flatnonzero((dig.cpu().numpy() != want).any(axis=1))
    assert bad.size == 0, f"AUTO, {n} x {L} B: {bad.size} digests differ, first {bad[:8].tolist()}"
    # which shape ran (csrc/sha1_runtime.hip split_unit; tests/test_gpu_dispatch.py has the whole table)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == 256 and LS.drain_cus() == 0, (cus, LS.drain_cus())
    assert launched == LS.expect(**{"quad" if n == 4096 else "unit4": 1}), f"AUTO, {n} chunks: launched {launched}"


@pytest.mark.parametrize("mode", list(MODES))
def test_initial_state(pkg, dev, monkeypatch, mode):
    """SHA1Update on contexts that already hold a non-IV state: the bulk of
    the second pieces runs in the quad shape from each context's own state
    (update mode: whole blocks, raw state out), 17 contexts, ragged pieces."""
    torch = dev
    set_env(monkeypatch, MODES[mode][1])
    rng = np.random.default_rng(17)
    n = 17
    first = [rng.integers(0, 256, 64 * (1 + i % 3), dtype=np.uint8) for i in range(n)]
    second = [rng.integers(0, 256, 64 * (i % 7) + 3 * i + 70, dtype=np.uint8) for i in range(n)]
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
