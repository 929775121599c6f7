"""Every path that answers "does this chunk have the expected SHA-1?" against
all 160 single-bit flips of the expected digest (tests/verdict_cases.py).

The library has seven compare implementations: the byte-wise compare kernel
(verify_batch DEVICE, the verify queue in batch mode, verify_gather), the
persistent drain's word-wise compare of the ring's `exp` slots, the two
progressive kernels' word-wise compare of the staged `expected` rows, the
backend's and the front end's host memcmp, and the hex strncmp of
verify_hash / verify_chunk_hash.  Each is reached here through its entry
points with the four cases of the builder -- the flip matrix in both
placements, swapped neighbour rows, inverted / zero / clean rows -- over 200
chunks of 0..700 bytes, and must answer exactly `mismatch` on all 200 rows:
"mismatch = 0" for a wrong digest is the one answer the library must never
give.  Where a path returns digests they are hashlib's whatever the verdict.
Expected-digest storage that is written again and again (a progressive
session's row, the drain's ring slots) is tested with alternating and rotated
expected values."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import launch_stats as ls
import verdict_cases as vc
from conftest import default_env
from test_gpu_parity import _run_verify, verify_driver  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
L512 = 524288
GUARD = 64
FILL = 0xAA
SEED = 160


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


@pytest.fixture(scope="module")
def ch():
    return vc.chunks(SEED)


@pytest.fixture(scope="module")
def cases(ch):
    return {name: vc.case(ch.want, name) for name in vc.CASES}


def _check(got, cases, ch, name, what):
    exp, mis = cases[name]
    vc.check(got, mis, exp, ch.want, f"{what}, {name}")


# ------------------------------------------------------- 1. verify_batch ----
@pytest.mark.parametrize("name", vc.CASES)
def test_verify_batch_host(pkg, dev, ch, cases, name):
    """flags HOST on the kernels: the backend's memcmp over the digests it
    copied back."""
    before = ls.snapshot()
    got = pkg.verify_batch(ch.data, ch.offsets, ch.lengths, cases[name][0])
    assert sum(ls.delta(before)[k] for k in ls.HASH) >= 1, "no kernel hashed the batch"
    _check(got, cases, ch, name, "verify_batch(HOST)")


@pytest.mark.parametrize("name", vc.CASES)
def test_verify_batch_device(pkg, dev, ch, cases, name):
    """flags DEVICE: the compare kernel; `expected` 4 bytes into its
    allocation, the mismatch buffer 0xAA before the call, its 64 guard bytes
    0xAA after."""
    torch = dev
    exp = cases[name][0]
    d_base = torch.from_numpy(np.array(ch.data)).cuda()
    d_off = torch.from_numpy(ch.offsets.astype(np.int64)).cuda()
    d_len = torch.from_numpy(ch.lengths.astype(np.int32)).cuda()
    raw = torch.zeros(4 + vc.N * 20, dtype=torch.uint8, device="cuda")
    d_exp = raw[4:]
    d_exp.copy_(torch.from_numpy(exp.reshape(-1)))
    mism = torch.full((vc.N + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pkg.sha1chunk.verify_batch_device(d_base, d_off, d_len, d_exp, mism, n=vc.N)
    got = mism.cpu().numpy()
    _check(got[:vc.N], cases, ch, name, "verify_batch(DEVICE)")
    assert (got[vc.N:] == FILL).all(), "bytes past n written"


_CHILD_HEAD = r"""
import importlib, json, os, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import verdict_cases as vc
pkg = importlib.import_module("congestion-control-with-bittorren_amd")
ch = vc.chunks(int(sys.argv[3]))
out = {}
"""

_ALL_DEVICES_CHILD = _CHILD_HEAD + r"""
assert pkg.device_count() == 2
for name in vc.CASES:
    exp, _ = vc.case(ch.want, name)
    out[name] = pkg.verify_batch(ch.data, ch.offsets, ch.lengths, exp, all_devices=True).tolist()
print("\nRESULT " + json.dumps(out))
"""


def _child(code, env, *args):
    r = subprocess.run([sys.executable, "-c", code, ROOT, TESTS, str(SEED)] + list(args), capture_output=True,
                       text=True, env=env, cwd=ROOT, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(line) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(line[0][7:])


@pytest.fixture(scope="module")
def all_devices_child(pkg, dev):
    """One child for the four cases: two logical devices on the one GPU, so
    the batch is sharded over two host threads and the verdicts are put
    together again."""
    return _child(_ALL_DEVICES_CHILD, dict(os.environ, SHA1CHUNK_VIRTUAL_DEVICES="2"))


@pytest.mark.parametrize("name", vc.CASES)
def test_verify_batch_all_devices(all_devices_child, ch, cases, name):
    _check(all_devices_child[name], cases, ch, name, "verify_batch(ALL_DEVICES)")


# ------------------------------------------------------ 2. verify_gather ----
@pytest.fixture(scope="module")
def segments(ch):
    """Every chunk as 1..4 segments of the packed buffer (an empty chunk as
    one empty segment), lengths cut at odd places."""
    rng = np.random.default_rng(SEED + 1)
    lists = []
    for i in range(vc.N):
        o, n = int(ch.offsets[i]), int(ch.lengths[i])
        k = min(1 + i % 4, max(n, 1))
        cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, n), k - 1, replace=False)) + [n] if k > 1 else [0, n]
        lists.append([(o + a, b - a) for a, b in zip(cuts, cuts[1:])])
        assert sum(L for _, L in lists[-1]) == n and len(lists[-1]) == k
    assert {len(m) for m in lists} == {1, 2, 3, 4}
    return lists


@pytest.fixture(scope="module")
def gather_stats(pkg):
    """s1be_gather_stats: [sub-batches, gather launches, messages skipped,
    calls from device / pinned / pageable memory]."""
    import ctypes as C
    be = ls.backend()
    be.s1be_gather_stats.restype = None
    be.s1be_gather_stats.argtypes = [C.POINTER(C.c_uint64), C.c_int]

    def read(reset=False):
        out = (C.c_uint64 * 6)()
        be.s1be_gather_stats(out, int(reset))
        return list(out)
    return read


@pytest.fixture(scope="module")
def pinned(pkg, dev, ch):
    buf = pkg.sha1chunk.pinned_alloc(ch.data.size)
    buf[:] = ch.data
    yield buf
    dev.cuda.synchronize()
    pkg.sha1chunk.pinned_free(buf)


@pytest.mark.parametrize("name", vc.CASES)
@pytest.mark.parametrize("source", ["pinned", "pageable"])
def test_verify_gather(pkg, dev, ch, cases, segments, gather_stats, pinned, source, name):
    """The compare kernel behind the gather: from a pinned base the device
    reads the segments in place, from a pageable one the host packs them."""
    base = pinned if source == "pinned" else np.array(ch.data)
    gather_stats(reset=True)
    got = pkg.sha1chunk.verify_gather(base, segments, cases[name][0])
    s = gather_stats()
    assert s[2] == 0 and s[3:] == {"pinned": [0, 1, 0], "pageable": [0, 0, 1]}[source], s
    _check(got, cases, ch, name, f"verify_gather({source})")
    assert np.array_equal(pkg.sha1chunk.hash_gather(base, segments), ch.want)


# ------------------------------------------------------- 3. verify queue ----
def _through_queue(q, ch, exp, how, rows=range(vc.N), tag0=0):
    """Rows `rows` of the case through the queue in that order, tag = tag0 +
    row; {tag: mismatch} of everything polled, each tag once."""
    held = []
    for i in rows:
        body = ch.chunk(i)
        if how == "submit":
            q.submit(body.tobytes(), exp[i].tobytes(), tag0 + i)
        else:
            r = q.reserve(body.size)
            r.view[:] = body
            q.commit(r, exp[i].tobytes(), tag0 + i)
            held.append((i, r))
    got = {}
    for tag, m in q.poll(wait=True, max_results=1 << 12):
        assert tag not in got, f"tag {tag} returned twice"
        got[tag] = m
    assert q.pending == 0 and q.poll() == []
    for i, r in held:  # the verify leaves the session's bytes alone
        assert np.array_equal(r.view, ch.chunk(i)), f"reserved buffer of row {i} changed"
        q.release(r)
    return got


def _verdicts(got, tag0=0):
    assert sorted(got) == [tag0 + i for i in range(vc.N)], "tags lost or invented"
    return np.array([got[tag0 + i] for i in range(vc.N)])


@pytest.mark.parametrize("name", vc.CASES)
@pytest.mark.parametrize("batch", [64, 24])
@pytest.mark.parametrize("how", ["submit", "reserve"])
@pytest.mark.parametrize("mode", ["persistent", "batch"])
def test_verify_queue(pkg, dev, monkeypatch, ch, cases, mode, how, batch, name):
    """The drain's compare of the ring's `exp` slots (persistent) and the
    compare kernel behind a batch launch (batch); batch = 24 closes groups
    below a wave's 64 lanes, 200 chunks leave a last group of 8."""
    monkeypatch.setenv("SHA1CHUNK_VQ_MODE", mode)
    before = ls.snapshot()
    with pkg.VerifyQueue(batch=batch, max_chunk_len=vc.MAX_LEN) as q:
        got = _through_queue(q, ch, cases[name][0], how)
    drains = ls.delta(before)["drain"]
    assert drains >= 1 if mode == "persistent" else drains == 0, drains
    _check(_verdicts(got), cases, ch, name, f"verify queue ({mode}, {how}, batch {batch})")


# --------------------------------------------- 4. verify queue, host path ----
_HOST_CHILD = _CHILD_HEAD + r"""
assert os.environ["SHA1CHUNK_HOST_SMALL"] == "4096"
for name in vc.CASES:
    exp, _ = vc.case(ch.want, name)
    for how in ("submit", "reserve"):
        got = {}
        with pkg.VerifyQueue(batch=1, max_chunk_len=vc.MAX_LEN) as q:
            for i in range(vc.N):
                body = ch.chunk(i)
                if how == "submit":
                    q.submit(body.tobytes(), exp[i].tobytes(), i)
                else:
                    r = q.reserve(body.size)
                    r.view[:] = body
                    q.commit(r, exp[i].tobytes(), i)
                    assert np.array_equal(r.view, body)
                    q.release(r)
                if i % 50 == 49:
                    for tag, m in q.poll():
                        assert tag not in got
                        got[tag] = m
            for tag, m in q.poll(wait=True):
                assert tag not in got
                got[tag] = m
            assert q.pending == 0
        assert sorted(got) == list(range(vc.N))
        out["vq " + how + " " + name] = [got[i] for i in range(vc.N)]
    # verify_batch(HOST) in slices of at most 4096 bytes: the front end's host route
    mis, lo = [], 0
    while lo < vc.N:
        hi = lo + 1
        while hi < vc.N and int(ch.lengths[lo:hi + 1].sum()) <= 4096:
            hi += 1
        assert int(ch.lengths[lo:hi].sum()) <= 4096
        mis += pkg.verify_batch(ch.data, ch.offsets[lo:hi], ch.lengths[lo:hi], exp[lo:hi]).tolist()
        lo = hi
    out["verify_batch " + name] = mis
# none of this started the HIP runtime
fds = [os.readlink(f"/proc/self/fd/{x}") for x in os.listdir("/proc/self/fd") if os.path.exists(f"/proc/self/fd/{x}")]
assert "/dev/kfd" not in fds, fds
print("\nRESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def host_child(pkg, dev):
    """One child under SHA1CHUNK_HOST_SMALL=4096 (the knob is read once per
    process): a verify queue of batch 1 and verify_batch(HOST) on batches of
    at most 4096 bytes hash on the host and compare with the front end's
    memcmp; the child never opens the device."""
    return _child(_HOST_CHILD, default_env(SHA1CHUNK_HOST_SMALL="4096"))


@pytest.mark.parametrize("name", vc.CASES)
@pytest.mark.parametrize("entry", ["vq submit", "vq reserve", "verify_batch"])
def test_front_end_host_route(host_child, ch, cases, entry, name):
    _check(host_child[f"{entry} {name}"], cases, ch, name, f"{entry} on the host route")


# ----------------------------------------------- 5. progressive verifier ----
def _wait(cond, what, timeout=20.0):
    t0 = time.perf_counter()
    while not cond():
        assert time.perf_counter() - t0 < timeout, f"timed out waiting for {what}"


def _mid_mark(n: int) -> int:
    """A mark inside a chunk of n >= 2 bytes that is no multiple of 64."""
    m = n // 2
    return m if m % 64 else m + 1


def _progressive(pkg, ch, exp, kernel, feeding, api):
    """All 200 chunks as concurrent sessions; ({tag: mismatch}, {tag:
    digest}, stats)."""
    with pkg.ProgressiveVerifier(sessions=vc.N, max_chunk_len=vc.MAX_LEN) as pv:
        rs = [pv.open(int(ch.lengths[i]), exp[i].tobytes(), i) for i in range(vc.N)]

        def advance(pairs):
            if api == "advance_many":
                assert pv.advance_many(pairs) == len(pairs)
            else:
                for r, mark in pairs:
                    pv.advance(r, mark)

        marks = [0] * vc.N
        if feeding == "split":  # the first launch stores a midstate (or has no whole block yet) ...
            for i, r in enumerate(rs):
                r.view[:] = vc.GUARD
                if r.length >= 2:
                    marks[i] = _mid_mark(r.length)
                    assert 0 < marks[i] < r.length and marks[i] % 64
                    r.view[:marks[i]] = ch.chunk(i)[:marks[i]]
            advance([(r, marks[i]) for i, r in enumerate(rs) if marks[i]])
            _wait(lambda: all(pv.hashed(r) >= (marks[i] & ~63) for i, r in enumerate(rs)), "the first marks' blocks")
            assert all(pv.hashed(r) == marks[i] & ~63 for i, r in enumerate(rs))
            assert pv.poll() == [] and any(pv.hashed(r) for r in rs)
        for i, r in enumerate(rs):  # ... the second resumes it and finishes
            r.view[marks[i]:] = ch.chunk(i)[marks[i]:]
        advance([(r, r.length) for r in rs])
        mis, dig = {}, {}
        for tag, m, d in pv.poll(wait=True, with_digests=True):
            assert tag not in mis, f"tag {tag} returned twice"
            mis[tag], dig[tag] = m, d
        assert pv.pending == 0 and pv.poll() == []
        st = pv.stats()
        for r in rs:
            pv.close(r)
    return mis, dig, st


@pytest.mark.parametrize("name", vc.CASES)
@pytest.mark.parametrize("api", ["advance", "advance_many"])
@pytest.mark.parametrize("feeding", ["whole", "split"])
@pytest.mark.parametrize("kernel", ["lane", "shared"])
def test_progressive(pkg, dev, monkeypatch, ch, cases, kernel, feeding, api, name):
    """Both progressive kernels' compare of the staged `expected` rows; a
    chunk that reaches its final block in its first launch, and one resumed
    from a stored midstate; one advance per session, and all 200 sessions
    in one advance_many call."""
    monkeypatch.setenv("SHA1CHUNK_PV_KERNEL", kernel)
    mis, dig, st = _progressive(pkg, ch, cases[name][0], kernel, feeding, api)
    assert st["kernel"] == kernel and st["launches"] >= 1
    assert st["launches_shared"] == (st["launches"] if kernel == "shared" else 0)
    wrong = [i for i in range(vc.N) if dig.get(i) != ch.want[i].tobytes()]
    assert not wrong, f"digests differ from hashlib at rows {wrong[:8]}"
    _check(_verdicts(mis), cases, ch, name, f"progressive ({kernel}, {feeding}, {api})")


# ------------------------------------------------------- 6. slot reuse ----
REUSE_BITS = (5, 44, 83, 122, 159, 31)  # words 0, 1, 2, 3, 4, 0


@pytest.mark.parametrize("kernel", ["lane", "shared"])
def test_progressive_session_reopened(pkg, dev, monkeypatch, ch, kernel):
    """One session, opened 12 times with the same data: its `expected` row
    is the true digest, then the digest with one bit flipped (each time
    another, of every word), in turn.  The kernel must read the row as it was
    written for this opening: verdicts 0, 1, 0, 1, ..."""
    monkeypatch.setenv("SHA1CHUNK_PV_KERNEL", kernel)
    row = 13  # 700 bytes
    data, want = ch.chunk(row), ch.want[row]
    assert data.size == vc.MAX_LEN and sorted({b // 32 for b in REUSE_BITS}) == [0, 1, 2, 3, 4]
    got, due = [], []
    with pkg.ProgressiveVerifier(sessions=1, max_chunk_len=vc.MAX_LEN) as pv:
        for k in range(12):
            exp = want.copy()
            if k % 2:
                bit = REUSE_BITS[k // 2]
                exp[bit // 8] ^= 1 << (bit % 8)
            t0 = time.perf_counter()
            while True:  # a closed session is held until its launches have completed
                try:
                    r = pv.open(data.size, exp.tobytes(), k)
                    break
                except pkg.Sha1ChunkError as e:
                    assert "in use" in str(e), e
                    assert time.perf_counter() - t0 < 20.0, "the session never came free"
            r.view[:] = data
            pv.advance(r, data.size)
            res = pv.poll(wait=True, with_digests=True)
            assert len(res) == 1 and res[0][0] == k and res[0][2] == want.tobytes(), res
            got.append(res[0][1])
            due.append(k % 2)
            pv.close(r)
        assert pv.stats()["kernel"] == kernel
    assert got == due, f"verdicts {got}: a reopened session answered for an earlier expected digest"


def test_drain_ring_slots_reused(pkg, dev, monkeypatch, ch, cases):
    """The persistent drain's `exp` ring slots written again.  The slot ring
    is never smaller than 512 slots (csrc/vq_persistent.hip: the data ring is
    at least 1 MiB and at least 128 chunks, a slot per quarter chunk); a 1 MiB
    ring and a maximal chunk length of 8 KiB give that size.  The stride flip
    matrix goes through one queue eight times back to back, 1600 submits, so
    every slot is written three or four times; three passes would reach only
    88 of the slots a second time.  Pass p starts at row 67 * p: the digest a
    slot held before is another row's, never the one due now (asserted below
    for 512 slots)."""
    monkeypatch.setenv("SHA1CHUNK_VQ_MODE", "persistent")
    monkeypatch.setenv("SHA1CHUNK_VQ_RING_MIB", "1")
    exp, mis = cases["stride"]
    passes, slots = 8, 512
    order = [[(i + 67 * p) % vc.N for i in range(vc.N)] for p in range(passes)]
    flat = [r for rows in order for r in rows]
    assert len(flat) >= 3 * slots
    assert all(not np.array_equal(exp[flat[k]], exp[flat[k - slots]]) for k in range(slots, len(flat)))
    before = ls.snapshot()
    with pkg.VerifyQueue(batch=64, max_chunk_len=8192) as q:
        got = [_through_queue(q, ch, exp, "submit", rows=order[p], tag0=1000 * p) for p in range(passes)]
    assert ls.delta(before)["drain"] >= 1
    for p in range(passes):
        vc.check(_verdicts(got[p], 1000 * p), mis, exp, ch.want, f"persistent queue, 512 slots, pass {p}")


# ------------------------------------------------------ 7. verify_hash ----
def _hex_cases(hexd: str):
    """[(what, hex string, verify_hash's answer)]: job.c:217-228 compares the
    strlen(calculated) = 40 lower-case characters it computed, as bytes."""
    rows = [("the digest", hexd, 0)]
    for pos in range(40):
        other = "0123456789abcdef"[(int(hexd[pos], 16) + 1 + pos % 15) % 16]
        assert other != hexd[pos]
        rows.append((f"character {pos} replaced", hexd[:pos] + other + hexd[pos + 1:], 1))
    assert hexd.upper() != hexd
    rows.append(("upper case", hexd.upper(), 1))
    rows.append(("characters behind the 40", hexd + "00ff", 0))
    return rows


@pytest.fixture(scope="module")
def big_chunk():
    import hashlib
    data = np.random.default_rng(SEED + 2).integers(0, 256, L512, dtype=np.uint8).tobytes()
    return data, hashlib.sha1(data).hexdigest()


def test_verify_hash_on_the_kernels(pkg, dev, big_chunk, capfd):
    data, hexd = big_chunk
    before = ls.snapshot()
    got = [(what, pkg.verify_hash(h, data)) for what, h, _ in _hex_cases(hexd)]
    capfd.readouterr()  # the reference's two lines per call
    assert sum(ls.delta(before)[k] for k in ls.HASH) >= 43, "every call hashes on a kernel"
    assert got == [(what, due) for what, _, due in _hex_cases(hexd)]


_VERIFY_HASH_CHILD = r"""
import importlib, json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
pkg = importlib.import_module("congestion-control-with-bittorren_amd")
assert "SHA1CHUNK_HOST_SMALL" not in os.environ
data = np.random.default_rng(int(sys.argv[3]) + 2).integers(0, 256, 524288, dtype=np.uint8).tobytes()
out = [pkg.verify_hash(h, data) for h in json.loads(sys.argv[4])]
# the host hashed: the HIP runtime was never started
fds = [os.readlink(f"/proc/self/fd/{x}") for x in os.listdir("/proc/self/fd") if os.path.exists(f"/proc/self/fd/{x}")]
assert "/dev/kfd" not in fds, fds
print("\nRESULT " + json.dumps(out))
"""


def test_verify_hash_default_routing(pkg, dev, big_chunk):
    """The same in a child without the suite's pin: the host hashes."""
    _, hexd = big_chunk
    rows = _hex_cases(hexd)
    got = _child(_VERIFY_HASH_CHILD, default_env(), json.dumps([h for _, h, _ in rows]))
    assert [(what, g) for (what, _, _), g in zip(rows, got)] == [(what, due) for what, _, due in rows]
    assert len(got) == 43


# ------------------------------------------------ 8. verify_chunk_hash ----
@pytest.fixture(scope="module")
def master_file(tmp_path_factory):
    """Nine whole chunks and a short tenth (above the 4 MiB host cut): (path,
    hex digests of the chunks, the last zero-padded to 512 KiB)."""
    import hashlib
    size = 9 * L512 + 1000
    data = np.random.default_rng(SEED + 3).integers(0, 256, size, dtype=np.uint8).tobytes()
    p = tmp_path_factory.mktemp("verdict") / "master.dat"
    p.write_bytes(data)
    padded = data + bytes(10 * L512 - size)
    return str(p), [hashlib.sha1(padded[i * L512:(i + 1) * L512]).hexdigest() for i in range(10)]


@pytest.mark.parametrize("pos", [None, 0, 20, 39], ids=["correct", "char0", "char20", "char39"])
@pytest.mark.parametrize("path", ["per-call", "master-index"])
def test_verify_chunk_hash(pkg, dev, verify_driver, master_file, path, pos):
    """chunk.c:204-217: returns on the right hex, exit(-1) with the
    reference's message on a hex with one character altered, in the first
    word, the middle and the last character.  Two right calls come first, so
    that the third is served from the master index where that is on."""
    file, hexes = master_file
    idx = 4
    hexd = hexes[idx]
    if pos is not None:
        hexd = hexd[:pos] + "0123456789abcdef"[(int(hexd[pos], 16) + 7) % 16] + hexd[pos + 1:]
        assert hexd != hexes[idx] and sum(a != b for a, b in zip(hexd, hexes[idx])) == 1
    r = _run_verify(verify_driver, file, [(9, hexes[9]), (1, hexes[1]), (idx, hexd)],
                    index=path == "master-index", settle_ms="0")
    assert r.stdout.count("the ascii of calculated hash is") == 3
    if pos is None:
        assert r.returncode == 0, r.stderr
        assert r.stdout.count("ok ") == 3 and "Unmatched" not in r.stderr
    else:
        assert r.returncode == 255, (r.returncode, r.stderr)
        assert f"Unmatched chunk hashes, requested hash {hexd}, calculated hash {hexes[idx]}" in r.stderr
        assert r.stdout.count("ok ") == 2
