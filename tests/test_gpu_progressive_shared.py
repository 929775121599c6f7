"""Progressive verification of many sessions at once (include/sha1chunk.h:
sha1chunk_burst_advance, sha1chunk_progress_stats, SHA1CHUNK_PV_KERNEL).
csrc/sha1_progress_shared.hip hashes a wave's 64 work-list entries with the
loads of each block step shared four lanes per entry and staged through LDS;
`SHA1CHUNK_PV_KERNEL=shared` sends every launch there, so small shapes reach
it: wave fill edges, unequal block counts around the five LDS buffers' wrap,
bytes above the mark, the 512 KiB stride, holes in the work list.  Expected
digests are hashlib's; the helpers are tests/test_gpu_progressive.py's."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from test_gpu_progressive import L512, LENGTHS, PKT, _bytes, _collect, _open, _wait, dev  # noqa: F401

pytestmark = pytest.mark.gpu


def _verifier(pkg, monkeypatch, kernel, sessions, max_chunk_len):
    """SHA1CHUNK_PV_KERNEL is read in create()."""
    if kernel is None:
        monkeypatch.delenv("SHA1CHUNK_PV_KERNEL", raising=False)
    else:
        monkeypatch.setenv("SHA1CHUNK_PV_KERNEL", kernel)
    return pkg.ProgressiveVerifier(sessions=sessions, max_chunk_len=max_chunk_len)


def _check_hashed(pv, r, mark, n):
    h = pv.hashed(r)
    assert h <= mark and (h % 64 == 0 or h == n), (h, mark, n)


def _feed_together(pv, rs, datas, step, garbage=True):
    """Every session one `step` further per advance_many, its bytes written
    just before; what is above the mark is not the chunk yet."""
    lens = [len(d) for d in datas]
    if garbage:
        for r in rs:
            r.view[:] = 0xA5
    marks = [0] * len(rs)
    live = list(range(len(rs)))
    while live:
        pairs = []
        for i in live:
            m = min(lens[i], marks[i] + step)
            rs[i].view[marks[i]:m] = datas[i][marks[i]:m]
            marks[i] = m
            pairs.append((rs[i], m))
        assert pv.advance_many(pairs) == len(pairs)
        for i in live:
            _check_hashed(pv, rs[i], marks[i], lens[i])
        live = [i for i in live if marks[i] < lens[i]]


@pytest.mark.parametrize("count", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130])
def test_wave_fill_edges(pkg, dev, monkeypatch, count):
    """1 .. 130 sessions (three waves, the last with 2 entries) on the shared
    kernel, every padding boundary among their lengths."""
    rng = np.random.default_rng(3000 + count)
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(count)]
    datas = [_bytes(rng, n) for n in lens]
    wants = [hashlib.sha1(d.tobytes()).digest() for d in datas]
    with _verifier(pkg, monkeypatch, "shared", count, 8192) as pv:
        rs = [pv.open(lens[i], wants[i], 100 + i) for i in range(count)]
        _feed_together(pv, rs, datas, PKT)
        got = _collect(pv, count)  # each tag once: _collect refuses a second
        assert got == {100 + i: (0, wants[i]) for i in range(count)}
        st = pv.stats()
        assert st["kernel"] == "shared" and st["launches_shared"] > 0
        assert st["launches_shared"] == st["launches"] and st["entries"] >= count
        assert pv.pending == 0 and pv.poll() == []
        for r in rs:
            pv.close(r)


def test_unequal_block_counts_in_one_wave(pkg, dev, monkeypatch):
    """One work list whose lanes have 0, 1, 2, 4, 5, 6 and 11 bulk blocks
    (below, at and beyond the five LDS buffers' wrap), final with tails 0, 1,
    55, 56 and 63 or not final; two more advances resume the rest from their
    stored midstates."""
    rng = np.random.default_rng(31)
    counts, tails = [0, 1, 2, 4, 5, 6, 11], [0, 1, 55, 56, 63]
    S = 64
    lens, plan = [], []
    for i in range(S):
        nb, kind = counts[i % 7], i % 8
        if kind < 5:  # final in the first work list
            n = 64 * nb + tails[kind]
            plan.append([n])
        else:  # two more advances: other block counts, then the tail
            more = counts[(i + kind) % 7]
            n = 64 * (nb + more + 3) + tails[(i + kind) % 5]
            plan.append([64 * nb + 13, 64 * (nb + more) + 50, n])
        lens.append(n)
    assert {(counts[i % 7], i % 8) for i in range(S)} >= {(c, k) for c in counts for k in range(8)}
    datas = [_bytes(rng, n) for n in lens]
    wants = [hashlib.sha1(d.tobytes()).digest() for d in datas]
    with _verifier(pkg, monkeypatch, "shared", S, max(lens)) as pv:
        rs = [pv.open(lens[i], wants[i], i) for i in range(S)]
        for r in rs:
            r.view[:] = 0x5A
        marks = [0] * S
        for step in range(3):
            pairs = []
            for i in range(S):
                if step < len(plan[i]):
                    m = plan[i][step]
                    rs[i].view[marks[i]:m] = datas[i][marks[i]:m]
                    marks[i] = m
                    pairs.append((rs[i], m))
            assert pv.advance_many(pairs) == len(pairs)
            for i in range(S):
                _check_hashed(pv, rs[i], marks[i], lens[i])
            if step == 0:  # the first call found both launch slots free: one work list
                assert pv.stats()["launches"] == 1 and pv.stats()["launches_shared"] == 1
            # the device catches up, so the next call's entries resume stored midstates
            _wait(lambda: all(pv.hashed(rs[i]) >= (marks[i] & ~63) for i in range(S) if marks[i] < lens[i]),
                  f"step {step}'s blocks")
            for i in range(S):
                _check_hashed(pv, rs[i], marks[i], lens[i])
        got = _collect(pv, S)
        assert got == {i: (0, wants[i]) for i in range(S)}
        assert all(pv.hashed(rs[i]) == lens[i] for i in range(S))
        for r in rs:
            pv.close(r)


def test_bytes_above_the_mark_are_not_read(pkg, dev, monkeypatch):
    """test_out_of_order_fill with 20 sessions on the shared kernel: garbage
    at and above every mark while launches run, the true bytes written just
    before the advance that covers them."""
    rng = np.random.default_rng(32)
    S, n = 20, 3 * PKT + 436
    datas = [_bytes(rng, n) for _ in range(S)]
    wants = [hashlib.sha1(d.tobytes()).digest() for d in datas]
    with _verifier(pkg, monkeypatch, "shared", S, n) as pv:
        rs = [pv.open(n, wants[i], 700 + i) for i in range(S)]
        mark = 0
        for upto in (PKT, 2 * PKT, n):
            for i, r in enumerate(rs):
                r.view[upto:] = _bytes(rng, n - upto)  # where later packets will land
                if upto == n:  # the later packets first
                    r.view[mark + PKT:upto] = datas[i][mark + PKT:upto]
                    r.view[mark:mark + PKT] = datas[i][mark:mark + PKT]
                else:
                    r.view[mark:upto] = datas[i][mark:upto]
            mark = upto
            assert pv.advance_many([(r, mark) for r in rs]) == S
            if mark < n:
                _wait(lambda: all(pv.hashed(r) >= (mark & ~63) for r in rs), f"the blocks below {mark}")
                assert all(pv.hashed(r) == mark & ~63 for r in rs)
        assert _collect(pv, S) == {700 + i: (0, wants[i]) for i in range(S)}
        assert pv.stats()["launches_shared"] == pv.stats()["launches"] > 0
        for r in rs:
            pv.close(r)


def test_large_stride(pkg, dev, monkeypatch, fixture_files, golden):
    """17 sessions 512 KiB apart (two load instructions' worth, the second
    with one live slot), the golden chunk in its 354 packets round-robin; one
    session's last packet and another's first carry a flipped bit."""
    chunk = np.frombuffer(fixture_files["tmp/C.tar"][:L512], np.uint8)
    want = bytes.fromhex(golden["fixtures"]["C.chunks_file"][0])
    assert hashlib.sha1(chunk.tobytes()).digest() == want
    S = 17
    datas = [chunk] * S
    bad_last, bad_first = chunk.copy(), chunk.copy()
    bad_last[L512 - 5] ^= 0x04
    bad_first[9] ^= 0x40
    datas[6], datas[16] = bad_last, bad_first
    with _verifier(pkg, monkeypatch, "shared", S, L512) as pv:
        rs = [pv.open(L512, want, 40 + i) for i in range(S)]
        _feed_together(pv, rs, datas, PKT, garbage=False)
        got = _collect(pv, S)
        expect = {40 + i: (0, want) for i in range(S)}
        expect[46] = (1, hashlib.sha1(bad_last.tobytes()).digest())
        expect[56] = (1, hashlib.sha1(bad_first.tobytes()).digest())
        assert got == expect
        st = pv.stats()
        assert st["launches_shared"] == st["launches"] > 0 and st["blocks"] == S * (L512 // 64)
        for r in rs:
            pv.close(r)


def test_holes_in_a_wave(pkg, dev, monkeypatch):
    """64 sessions, every third closed between two advance_many calls: the
    rest complete, the closed ones deliver nothing, and their slots, opened
    again, start from the IV."""
    rng = np.random.default_rng(34)
    S = 64
    lens = [int(x) for x in rng.integers(65, 8193, S)]
    datas = [_bytes(rng, n) for n in lens]
    wants = [hashlib.sha1(d.tobytes()).digest() for d in datas]
    with _verifier(pkg, monkeypatch, "shared", S, 8192) as pv:
        rs = [pv.open(lens[i], wants[i], i) for i in range(S)]
        for i, r in enumerate(rs):
            r.view[:] = datas[i]
        assert pv.advance_many([(rs[i], int(rng.integers(64, lens[i]))) for i in range(S)]) == S
        closed = [i for i in range(S) if i % 3 == 0]
        kept = [i for i in range(S) if i % 3 != 0]
        for i in closed:  # their launch may still be enqueued
            pv.close(rs[i])
        assert pv.advance_many([(rs[i], lens[i]) for i in kept]) == len(kept)
        assert _collect(pv, len(kept)) == {i: (0, wants[i]) for i in kept}
        assert pv.pending == 0
        again = {}
        new = []
        for j in range(len(closed)):
            n = int(rng.integers(65, 8193))
            d = _bytes(rng, n)
            again[1000 + j] = (0, hashlib.sha1(d.tobytes()).digest())
            r = _open(pkg, pv, n, again[1000 + j][1], 1000 + j)
            r.view[:] = d
            new.append((r, n))
        assert pv.advance_many([(r, n // 2) for r, n in new]) == len(new)
        assert pv.advance_many(new) == len(new)
        assert _collect(pv, len(new)) == again  # nothing of the closed sessions among them
        assert pv.pending == 0 and pv.poll() == []
        assert pv.stats()["launches_shared"] == pv.stats()["launches"]


def test_auto_routing(pkg, dev, monkeypatch):
    """auto: a lone session stays on the lane kernel; 64 sessions advanced
    together reach the shared one; `lane` forces the lane kernel on them, with
    the same results."""
    rng = np.random.default_rng(35)
    n = 3 * PKT + 436
    S = 64
    datas = [_bytes(rng, n) for _ in range(S)]
    wants = [hashlib.sha1(d.tobytes()).digest() for d in datas]
    bad = {5, 40}
    exps = [wants[i] if i not in bad else bytes([wants[i][0] ^ 1]) + wants[i][1:] for i in range(S)]

    with _verifier(pkg, monkeypatch, None, 2, n) as pv:
        assert pv.stats()["kernel"] == "auto"
        r = pv.open(n, wants[0], 1)
        mark = 0
        while mark < n:
            step = min(PKT, n - mark)
            r.view[mark:mark + step] = datas[0][mark:mark + step]
            mark += step
            pv.advance(r, mark)
            if mark < n:
                _wait(lambda: pv.hashed(r) >= (mark & ~63), f"hashed to reach {mark & ~63}")
        assert _collect(pv, 1) == {1: (0, wants[0])}
        st = pv.stats()
        assert st["launches"] >= 4 and st["launches_shared"] == 0
        pv.close(r)

    results = {}
    for kernel in (None, "shared", "lane"):
        with _verifier(pkg, monkeypatch, kernel, S, n) as pv:
            rs = [pv.open(n, exps[i], i) for i in range(S)]
            _feed_together(pv, rs, datas, PKT)
            results[kernel] = _collect(pv, S)
            st = pv.stats()
            if kernel == "lane":
                assert st["kernel"] == "lane" and st["launches"] > 0 and st["launches_shared"] == 0
            else:
                assert st["launches_shared"] > 0, st
            for r in rs:
                pv.close(r)
    assert results["shared"] == {i: (1 if i in bad else 0, wants[i]) for i in range(S)}
    assert results["lane"] == results["shared"] and results[None] == results["shared"]


def test_advance_many_semantics(pkg, dev, monkeypatch):
    """A refused pair in the middle: EINVAL, `applied` its index, the pairs
    before it in effect and those after it not; the same buffer twice with
    rising marks; n == 0; other sessions undisturbed."""
    rng = np.random.default_rng(36)
    E = pkg.sha1chunk.EINVAL
    L = pkg.lib()
    n = 6000
    datas = [_bytes(rng, n) for _ in range(4)]
    wants = [hashlib.sha1(d.tobytes()).digest() for d in datas]
    foreign = np.zeros(256, np.uint8)

    def burst(pv, pairs):
        k = len(pairs)
        bufs = (C.c_void_p * max(k, 1))(*[p for p, _ in pairs])
        marks = (C.c_uint32 * max(k, 1))(*[m for _, m in pairs])
        applied = C.c_size_t(99)
        rc = L.sha1chunk_burst_advance(pv._p, bufs, marks, k, C.byref(applied))
        return rc, applied.value

    with _verifier(pkg, monkeypatch, "shared", 4, n) as pv:
        a, b, c, d = [pv.open(n, wants[i], i) for i in range(4)]
        for i, r in enumerate((a, b, c, d)):
            r.view[:] = datas[i]
        pv.advance(d, 1000)  # the bystander
        pv.advance(b, 500)
        a_mark = 0
        for bad, text in (((foreign.ctypes.data, 80), b"not an open session"), ((b.ptr, 499), b"back"),
                          ((b.ptr, n + 1), b"beyond")):
            a_mark += 700
            assert burst(pv, [(a.ptr, a_mark), bad, (c.ptr, 3000)]) == (E, 1)
            assert text in L.sha1chunk_last_error(), L.sha1chunk_last_error()
            # the pair before it took effect and went to the device ...
            _wait(lambda: pv.hashed(a) >= (a_mark & ~63), f"a's blocks below {a_mark}")
            with pytest.raises(pkg.Sha1ChunkError):
                pv.advance(a, a_mark - 1)
            # ... the pair after it did not: c's mark is still 0 (1 would otherwise move it back)
            assert pv.hashed(c) == 0
        pv.advance(c, 1)
        with pytest.raises(pkg.Sha1ChunkError) as ei:  # the Python form: .applied
            pv.advance_many([(c, 100), (b, 400), (a, n)])
        assert ei.value.code == E and ei.value.applied == 1
        assert burst(pv, [(a.ptr, 2500), (a.ptr, 2600), (a.ptr, 2600), (a.ptr, n)]) == (0, 4)  # rising marks
        assert burst(pv, []) == (0, 0)
        assert L.sha1chunk_burst_advance(pv._p, None, None, 0, None) == 0  # a pump
        assert L.sha1chunk_burst_advance(pv._p, None, None, 1, None) == E
        assert burst(pv, [(a.ptr, n)]) == (E, 0)  # after completion, as advance()
        assert pv.advance_many([(b, n), (c, n), (d, n)]) == 3
        assert _collect(pv, 4) == {i: (0, wants[i]) for i in range(4)}
        assert pv.pending == 0
        for r in (a, b, c, d):
            pv.close(r)


def test_bad_kernel_name(pkg, dev, monkeypatch):
    monkeypatch.setenv("SHA1CHUNK_PV_KERNEL", "bogus")
    assert not pkg.lib().sha1chunk_pv_create(4, 4096)
    assert b"SHA1CHUNK_PV_KERNEL" in pkg.lib().sha1chunk_last_error()
    with pytest.raises(pkg.Sha1ChunkError) as ei:
        pkg.ProgressiveVerifier(sessions=4, max_chunk_len=4096)
    assert ei.value.code == pkg.sha1chunk.EINVAL and "SHA1CHUNK_PV_KERNEL" in str(ei.value)
    monkeypatch.setenv("SHA1CHUNK_PV_KERNEL", "lane")
    with pkg.ProgressiveVerifier(sessions=4, max_chunk_len=4096) as pv:
        assert pv.stats()["kernel"] == "lane" and pv.stats()["depth"] == 4
