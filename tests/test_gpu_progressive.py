"""Progressive chunk verification (sha1chunk_pv, include/sha1chunk.h): a
chunk is hashed on the device while it is received.  advance(buf, ready)
declares bytes [0, ready) final -- what cumulative_ack's last_packet_acked
says of recv_session->data (reliable_udp.c:300-324) -- and the kernel of
csrc/sha1_progress.hip resumes the session's midstate over the new whole
blocks; the verdict follows the last packet by the last <= 24 blocks, not by
the chunk's whole chain.

Expected digests are hashlib's; the full chunk is the committed C.tar fixture
with its golden digest."""
import hashlib
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L512 = 524288
PKT = 1484  # DATA payload bytes: 353 x 1484 + 436 = 512 KiB
LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 1484, 4097, 3 * 1484 + 436]
PATTERNS = ["one", "64", "1484", "random", "1"]


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def _steps(pattern, n, rng):
    if pattern == "one":
        return [n] if n else []
    if pattern == "random":
        out, left = [], n
        while left:
            s = int(rng.integers(1, min(left, 700) + 1))
            out.append(s)
            left -= s
        return out
    step = int(pattern)
    return [min(step, n - at) for at in range(0, n, step)]


def _wait(cond, what, timeout=20.0):
    t0 = time.perf_counter()
    while not cond():
        assert time.perf_counter() - t0 < timeout, f"timed out waiting for {what}"


def _collect(pv, n, timeout=20.0):
    """n results by non-blocking polls: {tag: (mismatch, digest)}."""
    got = {}

    def more():
        for tag, m, d in pv.poll(with_digests=True):
            assert tag not in got, f"tag {tag} returned twice"
            got[tag] = (m, d)
        return len(got) >= n
    _wait(more, f"{n} results", timeout)
    return got


def _feed(pv, r, data, steps, catch_up=False):
    """Write each step's bytes just before the advance that declares them
    final; `hashed` never passes the mark."""
    n, mark = len(data), 0
    for s in steps:
        r.view[mark:mark + s] = data[mark:mark + s]
        mark += s
        pv.advance(r, mark)
        h = pv.hashed(r)
        assert h <= mark and (h % 64 == 0 or h == n), (h, mark, n)
        if catch_up and mark < n:
            _wait(lambda: pv.hashed(r) >= (mark & ~63), f"hashed to reach {mark & ~63}")
            assert pv.hashed(r) == mark & ~63
    if not steps:
        pv.advance(r, 0)


def _open(pkg, pv, n, want, tag):
    """open(); while every session is in use -- a closed one is held until
    the launches that refer to it have completed, which open() itself checks
    -- try again."""
    t0 = time.perf_counter()
    while True:
        try:
            return pv.open(n, want, tag)
        except pkg.Sha1ChunkError as e:
            assert "in use" in str(e), e
            assert time.perf_counter() - t0 < 20.0, "no session came free"


@pytest.mark.parametrize("pattern", PATTERNS)
def test_boundary_lengths_and_feeding_patterns(pkg, dev, pattern):
    """Every padding boundary under every feeding pattern; on every other
    run the test lets the device catch up between advances, so launches of a
    single block (and, with 64-byte steps, two launches reading the two
    halves of one 128-byte line, the second written in between) occur."""
    rng = np.random.default_rng(1000 + PATTERNS.index(pattern))
    with pkg.ProgressiveVerifier(sessions=2, max_chunk_len=max(LENGTHS)) as pv:
        tag = 0
        for n in LENGTHS:
            if pattern == "1" and n > 129:
                continue
            for catch_up in (False, True):
                data = _bytes(rng, n)
                want = hashlib.sha1(data.tobytes()).digest()
                tag += 1
                r = _open(pkg, pv, n, want, tag)
                assert r.ptr % 128 == 0
                r.view[:] = 0xA5  # what is above the mark is not the chunk yet
                _feed(pv, r, data, _steps(pattern, n, rng), catch_up)
                got = _collect(pv, 1)
                assert got == {tag: (0, want)}, (pattern, n, catch_up)
                assert pv.hashed(r) == n
                pv.close(r)
        assert pv.pending == 0


def test_out_of_order_fill(pkg, dev):
    """Packets above the mark land in any order and may be overwritten: the
    device reads none of it before the mark passes."""
    rng = np.random.default_rng(2)
    n = 3 * PKT + 436
    data = _bytes(rng, n)
    want = hashlib.sha1(data.tobytes()).digest()
    with pkg.ProgressiveVerifier(sessions=1, max_chunk_len=n) as pv:
        r = pv.open(n, want, 7)
        r.view[:PKT] = data[:PKT]
        r.view[PKT:] = _bytes(rng, n - PKT)  # garbage where packets 1.. will land
        pv.advance(r, PKT)
        _wait(lambda: pv.hashed(r) >= (PKT & ~63), "the first packet's blocks")
        assert pv.hashed(r) == PKT & ~63
        r.view[2 * PKT:] = data[2 * PKT:]  # the later packets first
        r.view[PKT:2 * PKT] = data[PKT:2 * PKT]
        pv.advance(r, n)
        assert _collect(pv, 1) == {7: (0, want)}
        pv.close(r)


def test_full_chunk_is_hashed_before_its_last_packet(pkg, dev, fixture_files, golden):
    """C.tar's first 512 KiB chunk in its 354 DATA packets: before the last
    packet is fed the device has hashed everything below it."""
    chunk = np.frombuffer(fixture_files["tmp/C.tar"][:L512], np.uint8)
    want = bytes.fromhex(golden["fixtures"]["C.chunks_file"][0])
    sizes = [PKT] * 353 + [436]
    assert sum(sizes) == L512
    with pkg.ProgressiveVerifier(sessions=1, max_chunk_len=L512) as pv:
        r = pv.open(L512, want, 99)
        mark = 0
        for s in sizes[:-1]:
            r.view[mark:mark + s] = chunk[mark:mark + s]
            mark += s
            pv.advance(r, mark)
            assert pv.poll() == []
            assert pv.hashed(r) <= mark
        early = (L512 - 436) & ~63
        _wait(lambda: pv.hashed(r) >= early, "the chain below the last packet")
        assert pv.hashed(r) == early and pv.pending == 0
        r.view[mark:] = chunk[mark:]
        pv.advance(r, L512)
        assert pv.pending == 1
        assert _collect(pv, 1) == {99: (0, want)}
        assert pv.hashed(r) == L512 and pv.pending == 0
        pv.close(r)


def test_corruption_and_compare_width(pkg, dev):
    """One flipped bit anywhere in the data, or in any of the expected
    digest's five words, is a mismatch; the returned digest is that of the
    bytes received."""
    rng = np.random.default_rng(4)
    n = 3 * PKT + 436
    data = _bytes(rng, n)
    want = hashlib.sha1(data.tobytes()).digest()
    steps = _steps("1484", n, rng)
    with pkg.ProgressiveVerifier(sessions=2, max_chunk_len=n) as pv:
        # block 0, the block straddling the first step boundary, the last byte
        for tag, at in enumerate((5, PKT - 4, n - 1)):
            bad = data.copy()
            bad[at] ^= 0x10
            r = _open(pkg, pv, n, want, tag)
            _feed(pv, r, bad, steps, catch_up=True)
            assert _collect(pv, 1) == {tag: (1, hashlib.sha1(bad.tobytes()).digest())}, at
            pv.close(r)
        for word in range(5):
            exp = bytearray(want)
            exp[4 * word + word % 4] ^= 1 << word
            r = _open(pkg, pv, n, bytes(exp), 10 + word)
            _feed(pv, r, data, steps)
            assert _collect(pv, 1) == {10 + word: (1, want)}, word
            pv.close(r)
        r = _open(pkg, pv, n, want, 20)
        _feed(pv, r, data, steps)
        assert _collect(pv, 1) == {20: (0, want)}
        pv.close(r)


def test_many_ragged_sessions(pkg, dev):
    """300 concurrent sessions (two workgroups, the second partial) of
    lengths 0..8192 advanced in random interleaving: lanes of one wave have
    different block counts in every launch."""
    rng = np.random.default_rng(5)
    S = 300
    lens = [int(x) for x in rng.integers(0, 8193, S)]
    lens[:4] = [0, 8192, 63, 64]
    datas = [_bytes(rng, n) for n in lens]
    wants = [hashlib.sha1(d.tobytes()).digest() for d in datas]
    bad = set(int(x) for x in rng.choice(S, 20, replace=False))
    with pkg.ProgressiveVerifier(sessions=S, max_chunk_len=8192) as pv:
        rs = []
        for i in range(S):
            exp = wants[i] if i not in bad else bytes([wants[i][0] ^ 0x80]) + wants[i][1:]
            rs.append(pv.open(lens[i], exp, 5000 + i))
            rs[-1].view[:] = datas[i]
        marks = [0] * S
        live = list(range(S))
        while live:
            k = int(rng.integers(0, len(live)))
            i = live[k]
            marks[i] = min(lens[i], marks[i] + int(rng.integers(0, 3000)))
            pv.advance(rs[i], marks[i])
            assert pv.hashed(rs[i]) <= marks[i]
            if marks[i] == lens[i]:
                live[k] = live[-1]
                live.pop()
        got = {}
        for tag, m, d in pv.poll(wait=True, with_digests=True):
            assert tag not in got
            got[tag] = (m, d)
        assert got == {5000 + i: (1 if i in bad else 0, wants[i]) for i in range(S)}
        assert pv.pending == 0 and pv.poll() == []
        for r in rs:
            pv.close(r)


def test_slot_reuse_and_dropped_chunks(pkg, dev):
    """4 sessions, 40 chunks: a reused slot starts from the IV and its
    result is told from its previous occupant's; a chunk closed before
    completion, launches still enqueued, delivers nothing."""
    rng = np.random.default_rng(6)
    want, got = {}, {}
    with pkg.ProgressiveVerifier(sessions=4, max_chunk_len=20000) as pv:
        open_rs = []
        for c in range(40):
            n = int(rng.integers(65, 20001))
            data = _bytes(rng, n)
            d = hashlib.sha1(data.tobytes()).digest()
            if len(open_rs) == 4:  # results of the four in flight, then their slots
                for tag, (m, dg) in _collect(pv, sum(1 for _, t in open_rs if t in want)).items():
                    got[tag] = (m, dg)
                for r, _ in open_rs:
                    pv.close(r)
                open_rs = []
            r = _open(pkg, pv, n, d, c)
            r.view[:] = data
            if c % 3 == 1:  # dropped part-way, its launch still enqueued
                pv.advance(r, int(rng.integers(64, n)))
                pv.close(r)
                continue
            mark = 0
            for s in _steps("random", n, rng):
                mark += s
                pv.advance(r, mark)
            want[c] = (0, d)
            open_rs.append((r, c))
        for tag, (m, dg) in _collect(pv, len(open_rs)).items():
            got[tag] = (m, dg)
        assert got == want
        assert pv.pending == 0 and pv.poll() == []


def test_misuse_is_refused_without_disturbing_others(pkg, dev):
    rng = np.random.default_rng(7)
    E = pkg.sha1chunk.EINVAL
    L = pkg.lib()
    good = _bytes(rng, 5000)
    want = hashlib.sha1(good.tobytes()).digest()
    with pkg.ProgressiveVerifier(sessions=2, max_chunk_len=5000) as pv:
        a = pv.open(5000, want, 1)
        a.view[:] = good
        pv.advance(a, 2000)
        b = pv.open(100, want, 2)
        with pytest.raises(pkg.Sha1ChunkError) as ei:  # every session in use
            pv.open(10, want, 3)
        assert "in use" in str(ei.value)
        with pytest.raises(pkg.Sha1ChunkError) as ei:  # too long for a buffer
            pv.open(5001, want, 3)
        assert "5001" in str(ei.value)
        pv.advance(b, 70)
        assert L.sha1chunk_pv_advance(pv._p, b.ptr, 69) == E  # backward
        assert b"back" in L.sha1chunk_last_error()
        assert L.sha1chunk_pv_advance(pv._p, b.ptr, 101) == E  # beyond len
        assert L.sha1chunk_pv_advance(pv._p, b.ptr + 64, 80) == E  # not a session's buffer
        foreign = np.zeros(256, np.uint8)
        assert L.sha1chunk_pv_advance(pv._p, foreign.ctypes.data, 80) == E
        assert L.sha1chunk_pv_close(pv._p, foreign.ctypes.data) == E
        pv.advance(b, 70)  # the same mark again is fine
        pv.close(b)  # dropped
        assert L.sha1chunk_pv_advance(pv._p, b.ptr, 80) == E  # closed
        pv.advance(a, 5000)
        assert L.sha1chunk_pv_advance(pv._p, a.ptr, 5000) == E  # after completion
        assert _collect(pv, 1) == {1: (0, want)}
        pv.close(a)
        assert pv.pending == 0


def test_threads_share_one_object(pkg, dev):
    """4 receive threads, 16 chunks each, on one object; each polls and
    keeps its own tags, handing the others' to their owners."""
    T, N = 4, 16
    lock = threading.Lock()
    inbox = {t: {} for t in range(T)}
    errors = []
    with pkg.ProgressiveVerifier(sessions=2 * T, max_chunk_len=30000) as pv:
        def run(t):
            try:
                rng = np.random.default_rng(80 + t)
                for c in range(N):
                    n = int(rng.integers(0, 30001))
                    data = _bytes(rng, n)
                    d = hashlib.sha1(data.tobytes()).digest()
                    bad = c % 5 == 2
                    tag = 1000 * t + c
                    r = _open(pkg, pv, n, d if not bad else d[:19] + bytes([d[19] ^ 1]), tag)
                    _feed(pv, r, data, _steps("random", n, rng), catch_up=c % 4 == 0)

                    def mine():
                        res = pv.poll(with_digests=True)
                        with lock:
                            for g, m, dg in res:
                                assert g not in inbox[g // 1000]
                                inbox[g // 1000][g] = (m, dg)
                            return tag in inbox[t]
                    _wait(mine, f"tag {tag}")
                    assert inbox[t][tag] == (int(bad), d)
                    pv.close(r)
            except BaseException as e:  # noqa: BLE001 -- reported by the main thread
                errors.append(e)
        th = [threading.Thread(target=run, args=(t,)) for t in range(T)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors, errors
        assert all(len(inbox[t]) == N for t in range(T))
        assert pv.pending == 0


def test_latency_after_the_last_packet(pkg, dev, fixture_files, golden):
    """The point of the object: with the earlier packets hashed, the verdict
    follows the final advance by ~24 blocks plus launch and poll cost, where
    the verify queue starts its 8192-block chain at submit.  The bound is
    wide (0.5x) so that only "nothing was hashed early" fails it."""
    chunk_b = fixture_files["tmp/C.tar"][:L512]
    chunk = np.frombuffer(chunk_b, np.uint8)
    want = bytes.fromhex(golden["fixtures"]["C.chunks_file"][0])
    sizes = [PKT] * 353 + [436]
    early = (L512 - 436) & ~63

    def progressive(pv, tag):
        r = _open(pkg, pv, L512, want, tag)
        mark = 0
        for s in sizes[:-1]:
            r.view[mark:mark + s] = chunk[mark:mark + s]
            mark += s
            pv.advance(r, mark)
        _wait(lambda: pv.hashed(r) >= early, "the chain below the last packet")
        r.view[mark:] = chunk[mark:]
        t0 = time.perf_counter()
        pv.advance(r, L512)
        res = []
        while not res:
            res = pv.poll()
            assert time.perf_counter() - t0 < 20.0
        t1 = time.perf_counter()
        assert res == [(tag, 0)]
        pv.close(r)
        return t1 - t0

    def queued(q, tag):
        t0 = time.perf_counter()
        q.submit(chunk_b, want, tag)
        res = []
        while not res:
            res = q.poll()
            assert time.perf_counter() - t0 < 20.0
        t1 = time.perf_counter()
        assert res == [(tag, 0)]
        return t1 - t0

    with pkg.ProgressiveVerifier(sessions=2, max_chunk_len=L512) as pv:
        progressive(pv, 0)  # warm-up: the first launch loads the code object
        prog = sorted(progressive(pv, 1 + i) for i in range(5))
    with pkg.VerifyQueue(batch=256, max_chunk_len=L512) as q:
        queued(q, 0)
        lone = sorted(queued(q, 1 + i) for i in range(5))
    print(f"final advance -> verdict: progressive median {prog[2] * 1e3:.3f} ms {[round(x * 1e3, 3) for x in prog]}, "
          f"lone-chunk verify queue median {lone[2] * 1e3:.3f} ms {[round(x * 1e3, 3) for x in lone]}")
    assert prog[2] <= 0.5 * lone[2], (prog, lone)


# ---- every instantiation of the lane kernel (SHA1CHUNK_PV_DEPTH) -----------
# sha1_progress_kernel<DEPTH> keeps DEPTH blocks in flight per lane; where the
# three instantiations differ is the refill index min(k + j + DEPTH, last) and
# the mask live = k + j < nb, i.e. block counts below, at and just above the
# depth and its multiples.
DEPTH_BLOCKS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25]
DEPTH_TAILS = [0, 1, 55, 56, 63]
DEPTH_SESSIONS = 32
DEPTH_STRIDE = 2048


def _depth_shapes():
    """(whole blocks, tail bytes) of the 32 sessions: every block count, each
    with two different tails, every tail."""
    shapes = [(DEPTH_BLOCKS[i % 15], DEPTH_TAILS[(i + i // 15) % 5]) for i in range(DEPTH_SESSIONS)]
    assert {b for b, _ in shapes} == set(DEPTH_BLOCKS) and {t for _, t in shapes} == set(DEPTH_TAILS)
    assert max(64 * b + t for b, t in shapes) < DEPTH_STRIDE
    return shapes


@pytest.fixture(scope="module")
def depth_corpus():
    """The sessions' bytes and hashlib's digests of them, made once."""
    rng = np.random.default_rng(77)
    datas = [_bytes(rng, 64 * b + t) for b, t in _depth_shapes()]
    return datas, [hashlib.sha1(d.tobytes()).digest() for d in datas]


def _whole_buffer(r):
    """The session's whole buffer, beyond the chunk's length too."""
    import ctypes as C
    return np.ctypeslib.as_array(C.cast(r.ptr, C.POINTER(C.c_uint8)), shape=(DEPTH_STRIDE,))


@pytest.mark.parametrize("depth", [2, 4, 8])
def test_every_prefetch_depth(pkg, dev, monkeypatch, depth_corpus, depth):
    """The lane kernel at each prefetch depth: 32 sessions whose whole-block
    counts lie below, at and above the depth and its multiples (0 .. 25) with
    tails 0, 1, 55, 56 and 63, 0xA5 wherever the chunk's bytes are not final
    yet.  (a) all completed by one advance_many on an idle object: one launch
    of 32 entries, every block count in one wave; (b) two rounds, the first up
    to 1, D - 1, D or D + 1 blocks, so that a resumed midstate meets each
    refill edge too.  Digests and verdicts are hashlib's; one expected digest
    per feeding is corrupted and must be flagged."""
    monkeypatch.setenv("SHA1CHUNK_PV_KERNEL", "lane")
    monkeypatch.setenv("SHA1CHUNK_PV_DEPTH", str(depth))
    shapes = _depth_shapes()
    datas, wants = depth_corpus
    lens = [len(d) for d in datas]
    S = DEPTH_SESSIONS

    def open_all(pv, bad, tag0):
        rs = []
        for i in range(S):
            exp = wants[i] if i != bad else wants[i][:7] + bytes([wants[i][7] ^ 0x20]) + wants[i][8:]
            r = pv.open(lens[i], exp, tag0 + i)
            assert r.ptr % 128 == 0
            _whole_buffer(r)[:] = 0xA5
            rs.append(r)
        return rs

    def expect(bad, tag0):
        return {tag0 + i: (1 if i == bad else 0, wants[i]) for i in range(S)}

    # (a) one call, one launch, one wave
    with pkg.ProgressiveVerifier(sessions=S, max_chunk_len=DEPTH_STRIDE) as pv:
        st0 = pv.stats()
        assert st0["kernel"] == "lane" and st0["depth"] == depth and st0["launches"] == 0
        rs = open_all(pv, bad=13, tag0=100)
        for i, r in enumerate(rs):
            r.view[:] = datas[i]
        assert pv.advance_many([(rs[i], lens[i]) for i in range(S)]) == S
        st = pv.stats()
        assert st["launches"] == st0["launches"] + 1 and st["entries"] == st0["entries"] + S, (st0, st)
        assert st["launches_shared"] == 0 and st["depth"] == depth
        assert st["blocks"] == st0["blocks"] + sum(b for b, _ in shapes)
        assert _collect(pv, S) == expect(13, 100)
        assert all(pv.hashed(rs[i]) == lens[i] for i in range(S)) and pv.pending == 0
        for r in rs:
            pv.close(r)

    # (b) two rounds: the second resumes stored midstates
    with pkg.ProgressiveVerifier(sessions=S, max_chunk_len=DEPTH_STRIDE) as pv:
        rs = open_all(pv, bad=21, tag0=200)
        ks = [1, depth - 1, depth, depth + 1]
        first = [64 * min(ks[i % 4], shapes[i][0]) for i in range(S)]
        assert {min(ks[i % 4], shapes[i][0]) for i in range(S)} >= set(ks)
        one = [i for i in range(S) if first[i] > 0]
        two = [i for i in range(S) if not (first[i] > 0 and first[i] == lens[i])]  # not complete after round one
        assert len(one) == sum(1 for b, _ in shapes if b > 0)  # every session with a whole block
        for i in one:
            rs[i].view[:first[i]] = datas[i][:first[i]]
        assert pv.advance_many([(rs[i], first[i]) for i in one]) == len(one)
        _wait(lambda: all(pv.hashed(rs[i]) >= first[i] for i in one), "the first round's blocks")
        for i in two:
            assert pv.hashed(rs[i]) == first[i]
            rs[i].view[first[i]:] = datas[i][first[i]:]
        assert pv.advance_many([(rs[i], lens[i]) for i in two]) == len(two)
        assert _collect(pv, S) == expect(21, 200)
        st = pv.stats()
        assert st["launches_shared"] == 0 and st["depth"] == depth
        assert st["blocks"] == sum(b for b, _ in shapes)
        assert pv.pending == 0 and pv.poll() == []
        for r in rs:
            pv.close(r)


def test_bad_prefetch_depth(pkg, dev, monkeypatch):
    """SHA1CHUNK_PV_DEPTH is read in create(): 3 is no instantiation."""
    monkeypatch.setenv("SHA1CHUNK_PV_DEPTH", "3")
    assert not pkg.lib().sha1chunk_pv_create(4, 4096)
    assert b"SHA1CHUNK_PV_DEPTH" in pkg.lib().sha1chunk_last_error()
    with pytest.raises(pkg.Sha1ChunkError) as ei:
        pkg.ProgressiveVerifier(sessions=4, max_chunk_len=4096)
    assert ei.value.code == pkg.sha1chunk.EINVAL and "SHA1CHUNK_PV_DEPTH" in str(ei.value)
