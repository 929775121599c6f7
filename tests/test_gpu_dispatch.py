"""GPU: which kernel every call launches.

The dispatch code (csrc/sha1_runtime.hip choose_kernel, split_unit, use_mixed;
launch_split's two variants of unit 11; the CUs a persistent verify-queue
drain holds) is checked on the backend's launch counters (s1be_launch_stats,
read through launch_stats.py), not on digests alone: each test clears the
dispatch knobs, takes a counter delta around one call and compares the whole
delta, so "nothing else launched" is part of every assertion.  Digests are
compared with hashlib first, so a failure on the counters is a dispatch
failure with right digests.

Counter layout (csrc/sha1_kernels.h LaunchCounter), s1be_launch_stats out[12]:
  [0] lane  [1] fused  [2] split unit 1  [3] split unit 4
  [4] split unit 11, lane-per-chunk loads  [5] split unit 11, shared loads
  [6] quad (unit 416)  [7] study shape  [8] mixed  [9] length sort
  [10] persistent drain  [11] gauge, never reset: CUs held by drains

All inputs are tiny: uniform batches are 64-byte chunks of one buffer whose
hashlib digests are computed once."""
import hashlib

import numpy as np
import pytest

import launch_stats as LS

pytestmark = pytest.mark.gpu

L = 64


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


@pytest.fixture(scope="module")
def corpus(dev, cus):
    """128 CUs' worth + 1 chunks of 64 random bytes, back to back, on the host
    and on the device, with hashlib's digests (computed once, read only)."""
    n = 128 * cus + 1
    host = np.random.default_rng(416).integers(0, 256, n * L, dtype=np.uint8)
    raw = host.tobytes()
    want = np.frombuffer(b"".join(hashlib.sha1(raw[i * L:(i + 1) * L]).digest() for i in range(n)),
                         np.uint8).reshape(n, 20)
    want.setflags(write=False)
    off = dev.arange(n, dtype=dev.int64, device="cuda") * L
    lens = dev.full((n,), L, dtype=dev.int32, device="cuda")
    return host, dev.from_numpy(host).cuda(), off, lens, want


def run(pkg, torch, corpus, n, entry, kernel="auto"):
    """Hash the corpus' first n chunks through the uniform or the ragged
    device entry point; the counter delta of that call, digests checked."""
    _, d_host, d_off, d_len, want = corpus
    dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    before = LS.snapshot()
    if entry == "uniform":
        pkg.hash_uniform_device(d_host, L, n, dig, kernel=kernel)
    else:
        pkg.hash_device(d_host, d_off[:n], d_len[:n], dig, kernel=kernel)
    torch.cuda.synchronize()
    d = LS.delta(before)
    bad = np.flatnonzero((dig.cpu().numpy() != want[:n]).any(axis=1))
    assert bad.size == 0, f"{entry} n={n}: {bad.size} digests differ from hashlib, first {bad[:8].tolist()}"
    return d


def test_counters_reset_and_gauge(pkg, dev, corpus, monkeypatch):
    """reset zeroes the eleven counters after reading them; a null `out` only
    resets; the gauge is not a counter."""
    LS.clear_knobs(monkeypatch)
    run(pkg, dev, corpus, 1, "uniform")
    assert LS.snapshot(reset=True)[6] >= 1
    assert LS.snapshot()[:LS.GAUGE] == [0] * LS.GAUGE
    run(pkg, dev, corpus, 1, "uniform")
    LS.backend().s1be_launch_stats(None, 1)
    assert LS.snapshot()[:LS.GAUGE] == [0] * LS.GAUGE


# ---- AUTO's table -----------------------------------------------------------
def uniform_table(cus):
    return [(1, "quad"), (16, "quad"), (16 * cus, "quad"),
            (16 * cus + 1, "unit4"), (64 * cus, "unit4"),
            (64 * cus + 1, "unit11_lane"), (128 * cus, "unit11_lane"),
            (128 * cus + 1, "fused")]


def test_auto_uniform_table(pkg, dev, cus, corpus, monkeypatch):
    """Uniform entry point: the quad shape up to 16 chunks per CU, 4-block
    units up to one group of 64 per CU, the 8-wave shape with lane-per-chunk
    loads up to two, the fused kernel beyond; never a sort."""
    LS.clear_knobs(monkeypatch)
    assert LS.drain_cus() == 0, "a persistent verify queue of an earlier test still holds CUs"
    for n, shape in uniform_table(cus):
        d = run(pkg, dev, corpus, n, "uniform")
        print(f"uniform n={n}: {d}")
        assert d == LS.expect(**{shape: 1}), f"uniform AUTO, {n} chunks on {cus} CUs: want one {shape} launch"


def test_auto_ragged_table(pkg, dev, cus, corpus, monkeypatch):
    """Ragged entry point: no sort up to 64 chunks, one sort above; more
    groups of 64 than CUs go to the mixed kernel and nothing else."""
    LS.clear_knobs(monkeypatch)
    assert LS.drain_cus() == 0
    table = [(64, LS.expect(quad=1)), (65, LS.expect(sort=1, quad=1)), (130, LS.expect(sort=1, quad=1)),
             (64 * cus + 1, LS.expect(sort=1, mixed=1))]
    for n, want in table:
        d = run(pkg, dev, corpus, n, "ragged")
        print(f"ragged n={n}: {d}")
        assert d == want, f"ragged AUTO, {n} chunks on {cus} CUs"


def test_unit11_variants(pkg, dev, cus, corpus, monkeypatch):
    """Unit 11 loads lane-per-chunk only where the chunks lie back to back
    (no offset array, no order); offsets or an order give the shared loads."""
    n = 64 * cus + 1
    LS.clear_knobs(monkeypatch, SHA1CHUNK_MIXED="0")
    assert run(pkg, dev, corpus, n, "ragged") == LS.expect(sort=1, unit11_shared=1), "AUTO, mixed off"
    LS.clear_knobs(monkeypatch, SHA1CHUNK_SPLIT_UNIT="11")
    for m in (130, n):
        assert run(pkg, dev, corpus, m, "ragged", kernel="split") == LS.expect(unit11_shared=1), f"ragged, {m}"
        assert run(pkg, dev, corpus, m, "uniform", kernel="split") == LS.expect(unit11_lane=1), f"uniform, {m}"


# ---- forced knobs behind AUTO -----------------------------------------------
FORCED = [({"SHA1CHUNK_FORCE_KERNEL": "lane"}, "lane", "lane"),
          ({"SHA1CHUNK_FORCE_KERNEL": "fused"}, "fused", "fused"),
          ({"SHA1CHUNK_FORCE_KERNEL": "split"}, "quad", "quad"),  # 130 chunks: split's own rule picks the quad shape
          ({"SHA1CHUNK_SPLIT_UNIT": "1"}, "unit1", "unit1"),
          ({"SHA1CHUNK_SPLIT_UNIT": "4"}, "unit4", "unit4"),
          ({"SHA1CHUNK_SPLIT_UNIT": "11"}, "unit11_lane", "unit11_shared"),
          ({"SHA1CHUNK_SPLIT_UNIT": "416"}, "quad", "quad"),
          ({"SHA1CHUNK_FORCE_KERNEL": "split", "SHA1CHUNK_SPLIT_UNIT": "1"}, "unit1", "unit1")]


@pytest.mark.parametrize("env,uniform,ragged", FORCED, ids=["-".join(e[0].values()) for e in FORCED])
def test_forced_knobs(pkg, dev, corpus, monkeypatch, env, uniform, ragged):
    """SHA1CHUNK_FORCE_KERNEL and SHA1CHUNK_SPLIT_UNIT behind kernel="auto"
    launch exactly what they name (130 chunks; the ragged entry point sorts
    first, and the forced kernel reads the order)."""
    LS.clear_knobs(monkeypatch, **env)
    assert run(pkg, dev, corpus, 130, "uniform") == LS.expect(**{uniform: 1})
    assert run(pkg, dev, corpus, 130, "ragged") == LS.expect(sort=1, **{ragged: 1})


def test_forced_beyond_the_thresholds(pkg, dev, cus, corpus, monkeypatch):
    """The forced kernel also at a count where AUTO would pick another."""
    n = 128 * cus + 1  # AUTO: fused
    LS.clear_knobs(monkeypatch, SHA1CHUNK_FORCE_KERNEL="split", SHA1CHUNK_SPLIT_UNIT="416")
    assert run(pkg, dev, corpus, n, "uniform") == LS.expect(quad=1)
    LS.clear_knobs(monkeypatch, SHA1CHUNK_FORCE_KERNEL="split")
    assert run(pkg, dev, corpus, n, "uniform") == LS.expect(unit1=1), "split's own rule above two groups per CU"
    LS.clear_knobs(monkeypatch, SHA1CHUNK_FORCE_KERNEL="fused")
    assert run(pkg, dev, corpus, 1, "uniform") == LS.expect(fused=1)


def test_unbuilt_unit_launches_nothing(pkg, dev, corpus, monkeypatch):
    """SHA1CHUNK_SPLIT_UNIT=3 (an A/B-library shape) fails the call."""
    torch = dev
    LS.clear_knobs(monkeypatch, SHA1CHUNK_SPLIT_UNIT="3")
    dig = torch.zeros((130, 20), dtype=torch.uint8, device="cuda")
    for call in (lambda: pkg.hash_uniform_device(corpus[1], L, 130, dig, kernel="auto"),
                 lambda: pkg.hash_device(corpus[1], corpus[2][:130], corpus[3][:130], dig, kernel="split")):
        before = LS.snapshot()
        with pytest.raises(pkg.sha1chunk.Sha1ChunkError, match="split shape 3 is not in this library"):
            call()
        torch.cuda.synchronize()
        assert LS.delta(before) == LS.expect()
    assert not dig.cpu().numpy().any(), "a failed call wrote digests"


# ---- beside a persistent drain ----------------------------------------------
def test_quad_counts_only_free_cus(pkg, dev, cus, corpus, monkeypatch):
    """A persistent verify queue takes its CUs at creation; the quad shape,
    which needs a free CU per workgroup, counts only the rest.  Nothing is
    submitted: the drain itself never starts."""
    LS.clear_knobs(monkeypatch)
    for k in ("SHA1CHUNK_VQ_MODE", "SHA1CHUNK_VQ_CUS", "SHA1CHUNK_VQ_CU_BUDGET"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SHA1CHUNK_VQ_RING_MIB", "8")
    assert LS.drain_cus() == 0
    with pkg.VerifyQueue(batch=64, max_chunk_len=4096):
        h = LS.drain_cus()
        assert 0 < h < cus, f"a persistent queue holds {h} of {cus} CUs"
        free = cus - h
        assert run(pkg, dev, corpus, 16 * free, "uniform") == LS.expect(quad=1), f"{free} CUs free, 16 chunks each"
        assert run(pkg, dev, corpus, 16 * free + 1, "uniform") == LS.expect(unit4=1), "one chunk beyond the free CUs"
        assert run(pkg, dev, corpus, 16 * cus, "uniform") == LS.expect(unit4=1), "16 chunks per CU, drain's included"
        assert run(pkg, dev, corpus, 16 * free, "ragged") == LS.expect(sort=1, quad=1)
        assert run(pkg, dev, corpus, 16 * free + 1, "ragged") == LS.expect(sort=1, unit4=1)
        assert LS.drain_cus() == h
    assert LS.drain_cus() == 0, "a destroyed queue gives its CUs back"
    assert run(pkg, dev, corpus, 16 * cus, "uniform") == LS.expect(quad=1)


def test_persistent_drain_is_counted(pkg, dev, monkeypatch):
    """A chunk submitted to a persistent queue starts the drain kernel and no
    hash kernel."""
    LS.clear_knobs(monkeypatch)
    for k in ("SHA1CHUNK_VQ_MODE", "SHA1CHUNK_VQ_CUS", "SHA1CHUNK_VQ_CU_BUDGET"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SHA1CHUNK_VQ_RING_MIB", "8")
    chunk = bytes(range(200))
    before = LS.snapshot()
    with pkg.VerifyQueue(batch=64, max_chunk_len=4096) as q:
        q.submit(chunk, hashlib.sha1(chunk).digest(), 7)
        q.submit(chunk, hashlib.sha1(chunk + b"x").digest(), 8)
        q.flush()
        got = []
        while q.pending:
            got += q.poll(wait=True)
    d = LS.delta(before)
    assert sorted(got) == [(7, 0), (8, 1)]
    assert d["drain"] >= 1 and {**d, "drain": 0} == LS.expect(), d


# ---- the call sites behind AUTO ---------------------------------------------
def test_call_site_shahash(pkg, dev, monkeypatch):
    """One message on the kernels (the suite pins SHA1CHUNK_HOST_SMALL=0): a
    one-chunk host batch."""
    LS.clear_knobs(monkeypatch)
    msg = bytes(range(256)) * 3 + b"tail"
    before = LS.snapshot()
    got = pkg.shahash(msg)
    d = LS.delta(before)
    assert got == hashlib.sha1(msg).digest()
    assert d == LS.expect(quad=1)


def test_call_site_host_batch(pkg, dev, corpus, monkeypatch):
    """70 chunks from pageable host memory: sorted on the host, one slot."""
    LS.clear_knobs(monkeypatch)
    host, want = corpus[0], corpus[4]
    n = 70
    before = LS.snapshot()
    got = pkg.hash_batch(host[:n * L], np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32))
    d = LS.delta(before)
    assert np.array_equal(got, want[:n])
    assert d == LS.expect(quad=1)


def test_call_site_verify_queue_batches(pkg, dev, corpus, monkeypatch):
    """A batch-mode verify queue: 64 chunks, then flush.  How many launches
    the 64 make is the queue's business; each is the quad shape."""
    LS.clear_knobs(monkeypatch)
    monkeypatch.setenv("SHA1CHUNK_VQ_MODE", "batch")
    host, want = corpus[0], corpus[4]
    n = 64
    wrong = {5, 63}
    before = LS.snapshot()
    with pkg.VerifyQueue(batch=256, max_chunk_len=4096) as q:
        assert LS.drain_cus() == 0, "a batch-mode queue holds no CUs"
        for i in range(n):
            exp = want[i].tobytes() if i not in wrong else want[i + 1].tobytes()
            q.submit(host[i * L:(i + 1) * L].tobytes(), exp, i)
        q.flush()
        got = []
        while q.pending:
            got += q.poll(wait=True)
    d = LS.delta(before)
    assert sorted(got) == [(i, int(i in wrong)) for i in range(n)]
    assert d["quad"] >= 1 and {**d, "quad": 0} == LS.expect(), d


def test_call_site_file_pipeline(pkg, dev, tmp_path, monkeypatch):
    """hash_fd on a file just over 4 MiB: nine chunks of 512 KiB, in as many
    slots as the pipeline cuts; each slot's launch is the quad shape."""
    LS.clear_knobs(monkeypatch)
    data = np.random.default_rng(9).integers(0, 256, (4 << 20) + 1000, dtype=np.uint8).tobytes()
    p = tmp_path / "just_over_4mib.bin"
    p.write_bytes(data)
    before = LS.snapshot()
    got = pkg.make_chunks(str(p))
    d = LS.delta(before)
    step = pkg.sha1chunk.CHUNK_LEN
    assert got == [hashlib.sha1(data[i:i + step]).digest() for i in range(0, len(data), step)] and len(got) == 9
    assert d["quad"] >= 1 and {**d, "quad": 0} == LS.expect(), d


def test_call_site_update_bulk(pkg, dev, monkeypatch):
    """Batched SHA1Update over 17 contexts: one bulk launch per call (the
    init, pre, post and final kernels are not hash kernels)."""
    torch = dev
    LS.clear_knobs(monkeypatch)
    rng = np.random.default_rng(17)
    n = 17
    pieces = [rng.integers(0, 256, 70 + 13 * i, dtype=np.uint8) for i in range(n)]
    lens = np.array([len(p) for p in pieces], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens.astype(np.uint64) + 3)[:-1]
    host = np.zeros(int(off[-1] + lens[-1]) + 64, np.uint8)
    for p, o in zip(pieces, off):
        host[int(o):int(o) + len(p)] = p
    ctx = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    d_host, d_off, d_len = (torch.from_numpy(host).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
                            torch.from_numpy(lens.astype(np.int32)).cuda())
    before = LS.snapshot()
    pkg.init_contexts_device(ctx, n=n, n_contexts=n)
    pkg.update_contexts_device(ctx, d_host, d_off, d_len, n=n, n_contexts=n)
    pkg.final_contexts_device(ctx, dig, n=n, n_contexts=n)
    torch.cuda.synchronize()
    d = LS.delta(before)
    got = dig.cpu().numpy()
    for i in range(n):
        assert got[i].tobytes() == hashlib.sha1(pieces[i].tobytes()).digest(), f"context {i}"
    assert d == LS.expect(quad=1)


@pytest.mark.parametrize("source", ["device", "pageable"])
def test_call_site_gather(pkg, dev, source, monkeypatch):
    """hash_gather_batch of five messages of one to three segments (an empty
    message among them): one sub-batch, one quad launch."""
    torch = dev
    LS.clear_knobs(monkeypatch)
    base = np.random.default_rng(5).integers(0, 256, 8192, dtype=np.uint8)
    messages = [[(100, 60), (4000, 150)], [(7, 1)], [], [(300, 64), (364, 64), (1000, 1)], [(5000, 3000)]]
    want = [hashlib.sha1(b"".join(base[o:o + n].tobytes() for o, n in m)).digest() for m in messages]
    src = torch.from_numpy(base).cuda() if source == "device" else base
    before = LS.snapshot()
    got = pkg.sha1chunk.hash_gather(src, messages)
    d = LS.delta(before)
    assert [g.tobytes() for g in got] == want
    assert d == LS.expect(quad=1)
