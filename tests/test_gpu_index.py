"""GPU: the digest index (include/sha1chunk.h, "Digest index";
csrc/sha1_index.hip, rt_index.hip).  Exact: every answer against a Python
dict of the table (lowest position, or NO_MATCH), guards around every id
array."""
import ctypes as C
import hashlib
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5A5A5A5
NO_MATCH = 0xFFFFFFFF
EINVAL, EALIGN = -1, -5
HOST, DEVICE = 0, 1
CHUNK = 524288
CHAIN_SEED = 20261020  # tools/index_map_check prints its prefixes' homes (tests/test_index_cpu.py)
TAIL = 8               # guard words behind every id array


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


@pytest.fixture(scope="module")
def backend(pkg):
    """The backend library itself: s1be_index_stats and the backend's own
    refusals, which the front end's checks never let through."""
    pkg.lib()
    be = C.CDLL(os.path.join(os.path.dirname(pkg.sha1chunk.LIB_PATH), "libsha1chunk_hip.so"))
    be.s1be_index_stats.restype = C.c_int
    be.s1be_index_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    be.s1be_index_lookup_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    be.s1be_index_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    be.s1be_match_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint]
    be.s1be_last_error.restype = C.c_char_p
    return be


def index_stats(backend, ix):
    """[slots, longest build probe, entries whose digest was in place, entries
    whose probe wrapped]."""
    out = (C.c_uint64 * 4)()
    assert backend.s1be_index_stats(ix._ix, out) == 0
    return list(out)


def digests(rng, n):
    return rng.integers(0, 256, (n, 20), dtype=np.uint8)


def lowest(table):
    """digest bytes -> lowest position."""
    d = {}
    for p, row in enumerate(table):
        d.setdefault(row.tobytes(), p)
    return d


def want_ids(d, queries):
    return np.array([d.get(q.tobytes(), NO_MATCH) for q in queries], np.uint32)


def off16(rows):
    """A copy of an (n, 20) uint8 array at an address that is 4 mod 16."""
    buf = np.zeros(rows.size + 32, np.uint8)
    at = (4 - buf.ctypes.data) % 16
    view = buf[at:at + rows.size].reshape(-1, 20)
    view[:] = rows
    assert (buf.ctypes.data + at) % 16 == 4 and (rows.size == 0 or view.ctypes.data == buf.ctypes.data + at)
    return view


def dev_off16(torch, rows):
    """The same on the device: (tensor, address), the address 4 mod 16."""
    t = torch.zeros(rows.size + 32, dtype=torch.uint8, device="cuda")
    at = (4 - t.data_ptr()) % 16
    t[at:at + rows.size] = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)).cuda()
    return t, t.data_ptr() + at


def host_lookup(pkg, ix, queries, n=None):
    """sha1chunk_index_lookup into a guarded id array -> the n ids."""
    n = queries.shape[0] if n is None else n
    q = off16(queries)
    ids = np.full(n + TAIL, GUARD, np.uint32)
    rc = pkg.lib().sha1chunk_index_lookup(ix._ix, q.ctypes.data, n, ids.ctypes.data)
    assert rc == 0, pkg.lib().sha1chunk_last_error()
    assert (ids[n:] == GUARD).all()
    return ids[:n]


def device_lookup(pkg, torch, ix, queries, n=None):
    n = queries.shape[0] if n is None else n
    keep, addr = dev_off16(torch, queries)
    ids = torch.from_numpy(np.full(n + TAIL, GUARD, np.uint32).view(np.int32)).cuda()
    rc = pkg.lib().sha1chunk_index_lookup_device_async(ix._ix, addr, n, ids.data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, pkg.lib().sha1chunk_last_error()
    torch.cuda.synchronize()
    got = ids.cpu().numpy().view(np.uint32)
    assert (got[n:] == GUARD).all()
    return got[:n]


# ----------------------------------------------------- 1. reference fixtures --
def test_reference_fixtures(tmp_path, pkg, dev, golden, fixture_files):
    hashes = golden["fixtures"]["C.chunks_file"]
    paths = {}
    for name, data in fixture_files.items():
        paths[name] = tmp_path / name.replace("/", "_")
        paths[name].write_bytes(data)
    with pkg.DigestIndex([bytes.fromhex(h) for h in hashes]) as ix:
        assert ix.size == 4 and len(ix) == 4
        assert ix.match_fd(paths["tmp/B.tar"]).tolist() == [2, 3]
        assert ix.match_fd(paths["tmp/A.tar"]).tolist() == [0, 1]
        assert ix.match_fd(paths["tmp/C.tar"]).tolist() == [0, 1, 2, 3]
        assert ix.match_fd(paths["example/A.gif"]).tolist() == [NO_MATCH, NO_MATCH]
        # from the fd's offset on, and the fd left where sha1chunk_hash_fd leaves it
        L = pkg.lib()
        fd, fd2 = os.open(paths["tmp/C.tar"], os.O_RDONLY), os.open(paths["tmp/C.tar"], os.O_RDONLY)
        try:
            os.lseek(fd, CHUNK, os.SEEK_SET)
            os.lseek(fd2, CHUNK, os.SEEK_SET)
            ids = np.full(2 + TAIL, GUARD, np.uint32)
            dig = np.zeros((2, 20), np.uint8)
            total, total2 = C.c_size_t(0), C.c_size_t(0)
            assert L.sha1chunk_match_fd(ix._ix, fd, ids.ctypes.data, 2, C.byref(total)) == 2
            assert L.sha1chunk_hash_fd(fd2, dig.ctypes.data_as(C.POINTER(C.c_uint8)), 2, C.byref(total2)) == 2
            assert ids[:2].tolist() == [1, 2] and (ids[2:] == GUARD).all()
            assert total.value == total2.value == 3
            assert os.lseek(fd, 0, os.SEEK_CUR) == os.lseek(fd2, 0, os.SEEK_CUR) == len(fixture_files["tmp/C.tar"])
        finally:
            os.close(fd)
            os.close(fd2)
    # the has-chunks file of B.tar under the master list, written in the
    # reference's form: header and chunk 0 on one line, CRLF line ends
    master = tmp_path / "C.masterchunks"
    master.write_bytes(("\r\n".join([f"File: /tmp/C.tar Chunks:0 {hashes[0]}"] +
                                    [f"{i} {h}" for i, h in enumerate(hashes) if i]) + "\r\n").encode())
    have = pkg.has_chunks(paths["tmp/B.tar"], master)
    assert have == [(2, bytes.fromhex(hashes[2])), (3, bytes.fromhex(hashes[3]))]
    assert have == [(i, bytes.fromhex(h)) for i, h in zip((2, 3), golden["fixtures"]["make_chunks"]["tmp/B.tar"])]
    assert pkg.has_chunks(paths["example/A.gif"], master) == []


# --------------------------------------------------------- 2. against a dict --
@pytest.mark.parametrize("m", [0, 1, 2, 3, 63, 64, 65, 1000, 70000])
def test_against_a_dict(pkg, dev, backend, m):
    torch = dev
    rng = np.random.default_rng(100 + m)
    table = digests(rng, m)
    d = lowest(table)
    hits = table[rng.permutation(m)]
    misses = digests(rng, max(50, m // 10))
    flips = np.zeros((0, 20), np.uint8)
    if m:
        # every single-bit flip of one present digest: a compare that skips a
        # word, or a byte of one, answers its position for some of these
        one = table[m // 2]
        flips = np.repeat(one[None, :], 160, axis=0)
        flips[np.arange(160), np.arange(160) // 8] ^= (1 << (np.arange(160) % 8)).astype(np.uint8)
    queries = np.concatenate([hits, misses, flips])
    queries = queries[rng.permutation(queries.shape[0])]
    want = want_ids(d, queries)
    assert (want != NO_MATCH).sum() == m
    # the table from host memory and, built again, from device memory, both 4 mod 16
    keep, addr = dev_off16(torch, table)
    torch.cuda.synchronize()
    for ix in (pkg.DigestIndex(off16(table)), pkg.DigestIndex(_Raw(addr, True), m)):
        with ix:
            assert ix.size == m
            st = index_stats(backend, ix)
            assert st[0] == max(8, 1 << (2 * m - 1).bit_length()) and st[0] >= 2 * m
            assert st[2] == 0 and (st[1] >= 1) == (m > 0)
            assert np.array_equal(host_lookup(pkg, ix, queries), want)
            assert np.array_equal(device_lookup(pkg, torch, ix, queries), want)
            # n = 0 leaves the ids alone
            assert (host_lookup(pkg, ix, queries, n=0).size, device_lookup(pkg, torch, ix, queries, n=0).size) == (0, 0)
            assert np.array_equal(ix.lookup(queries[:7]), want[:7])


class _Raw:
    """A bare address posing as a tensor for DigestIndex."""

    def __init__(self, addr, is_cuda):
        self.addr, self.is_cuda = addr, is_cuda

    def data_ptr(self):
        return self.addr


# ------------------------------------------------------------ 3. duplicates --
def test_duplicates_lowest_position_wins(pkg, dev, backend):
    torch = dev
    rng = np.random.default_rng(3)
    base = digests(rng, 500)
    zero = np.frombuffer(hashlib.sha1(bytes(CHUNK)).digest(), np.uint8)  # a sparse file's all-zero chunk
    rows = np.concatenate([np.repeat(base, rng.integers(1, 6, 500), axis=0), np.repeat(zero[None, :], 4096, axis=0)])
    table = rows[rng.permutation(rows.shape[0])]
    m = table.shape[0]
    d = lowest(table)
    assert len(d) == 501
    queries = np.concatenate([base, zero[None, :], table[rng.permutation(m)[:700]], digests(rng, 100)])
    want = want_ids(d, queries)
    with pkg.DigestIndex(table) as ix:
        assert np.array_equal(host_lookup(pkg, ix, queries), want)
        assert np.array_equal(device_lookup(pkg, torch, ix, queries), want)
        assert index_stats(backend, ix)[2] == m - 501


# ---------------------------------------------------------------- 4. chains --
def _splitmix64(x):
    M = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def test_chains_of_one_home(pkg, dev, backend):
    """200 distinct digests that share their first 8 bytes share a home slot:
    one chain of 200 in 512 slots, which wraps for the prefixes whose home is
    among the last slots (tools/index_map_check lists them for CHAIN_SEED)."""
    torch = dev
    rng = np.random.default_rng(4)
    wrapped = 0
    for k in range(32):
        prefix = np.frombuffer(_splitmix64(CHAIN_SEED + k).to_bytes(8, "little"), np.uint8)
        rows = digests(rng, 250)
        rows[:, :8] = prefix
        assert len({r.tobytes() for r in rows}) == 250
        table, misses = rows[:200], rows[200:]
        d = lowest(table)
        queries = np.concatenate([table[rng.permutation(200)], misses])
        want = want_ids(d, queries)
        assert (want[200:] == NO_MATCH).all()
        with pkg.DigestIndex(table) as ix:
            st = index_stats(backend, ix)
            assert st[0] == 512 and st[1] >= 200 and st[2] == 0, (k, st)
            wrapped += st[3]
            got = device_lookup(pkg, torch, ix, queries) if k % 2 else host_lookup(pkg, ix, queries)
            assert np.array_equal(got, want), k
    assert wrapped > 0


def test_tiny_tables(pkg, dev):
    """200 random tables of 3 or 4 digests in 8 slots: collisions and wraps at
    the smallest array."""
    rng = np.random.default_rng(5)
    for t in range(200):
        table = digests(rng, 3 + t % 2)
        if t % 5 == 0:
            table[2] = table[0]
        queries = np.concatenate([table, digests(rng, 4)])
        with pkg.DigestIndex(table) as ix:
            assert np.array_equal(ix.lookup(queries), want_ids(lowest(table), queries)), t


# ------------------------------- 5. one stream, no host synchronise between --
def test_hash_then_lookup_on_one_stream(pkg, dev, oracle):
    torch = dev
    rng = np.random.default_rng(6)
    n, L = 64, 4096
    host = oracle.synth_chunks(0, n, L)
    dig = oracle.hash_batch(host, np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32))
    perm = rng.permutation(n)
    inverse = np.argsort(perm)  # table[j] = dig[perm[j]]: chunk i is at position inverse[i]
    s = torch.cuda.Stream()
    with pkg.DigestIndex(dig[perm]) as ix, torch.cuda.stream(s):
        buf = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        d_dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
        ids = torch.from_numpy(np.full(n + TAIL, GUARD, np.uint32).view(np.int32)).cuda()
        pkg.synth_fill_device(buf, 0, n, L, stream=s)
        pkg.hash_uniform_device(buf, L, n, d_dig, stream=s)
        ix.lookup_device(d_dig, ids, n=n, stream=s)
        s.synchronize()
        got = ids.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:n], inverse.astype(np.uint32)) and (got[n:] == GUARD).all()
    # ragged chunks, a zero-length one among them, through sha1chunk_hash_device_async
    lengths = np.array([0, 1, 55, 56, 63, 64, 65, 119, 120, 1000, 4096, 70001] + list(rng.integers(1, 9000, 60)),
                       np.uint32)
    n = lengths.size
    off, total = pkg.sha1chunk.ragged_layout(lengths, 8)
    data = rng.integers(0, 256, max(total, 8), dtype=np.uint8)
    dig = np.array([np.frombuffer(hashlib.sha1(data[o:o + l].tobytes()).digest(), np.uint8)
                    for o, l in zip(off.tolist(), lengths.tolist())])
    assert len({r.tobytes() for r in dig}) == n
    perm = rng.permutation(n)
    inverse = np.argsort(perm)
    with pkg.DigestIndex(dig[perm]) as ix, torch.cuda.stream(s):
        base = torch.from_numpy(data).cuda()
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        d_len = torch.from_numpy(lengths.view(np.int32)).cuda()
        d_dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
        ids = torch.from_numpy(np.full(n + TAIL, GUARD, np.uint32).view(np.int32)).cuda()
        pkg.hash_device(base, d_off, d_len, d_dig, stream=s)
        ix.lookup_device(d_dig, ids, n=n, stream=s)
        s.synchronize()
        got = ids.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:n], inverse.astype(np.uint32)) and (got[n:] == GUARD).all()


# ----------------------------------------------------------- 6. match_batch --
def test_match_batch_host_and_device(pkg, dev):
    torch = dev
    rng = np.random.default_rng(7)
    lengths = np.array([0, 1, 64, 65, 4095, 4096, 150000] + list(rng.integers(1, 20000, 83)), np.uint32)
    n = lengths.size
    off, total = pkg.sha1chunk.ragged_layout(lengths, 8)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    dig = np.array([np.frombuffer(hashlib.sha1(data[o:o + l].tobytes()).digest(), np.uint8)
                    for o, l in zip(off.tolist(), lengths.tolist())])
    listed = np.array([i for i in range(n) if i % 3 != 0])  # every third chunk is absent from the index
    listed = listed[rng.permutation(listed.size)]
    want = np.full(n, NO_MATCH, np.uint32)
    want[listed] = np.arange(listed.size)
    with pkg.DigestIndex(dig[listed]) as ix:
        assert np.array_equal(ix.match_batch(data, off, lengths), want)
        ids = torch.from_numpy(np.full(n + TAIL, GUARD, np.uint32).view(np.int32)).cuda()
        ix.match_batch(torch.from_numpy(data).cuda(), torch.from_numpy(off.view(np.int64)).cuda(),
                       torch.from_numpy(lengths.view(np.int32)).cuda(), ids)
        got = ids.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:n], want) and (got[n:] == GUARD).all()
        assert ix.match_batch(data, [], []).size == 0


# ---------------------------------------------------- 7. concurrent lookups --
def test_concurrent_host_lookups(pkg, dev):
    rng = np.random.default_rng(8)
    table = digests(rng, 5000)
    table[rng.integers(0, 5000, 300)] = table[:300]  # some duplicates
    d = lowest(table)
    pool = np.concatenate([table, digests(rng, 2000)])
    L = pkg.lib()
    errors = []

    def worker(t, ix):
        r = np.random.default_rng(80 + t)
        try:
            for call in range(200):
                n = int(r.integers(1, 301))
                q = np.ascontiguousarray(pool[r.integers(0, pool.shape[0], n)])
                ids = np.full(n + TAIL, GUARD, np.uint32)
                rc = L.sha1chunk_index_lookup(ix._ix, q.ctypes.data, n, ids.ctypes.data)
                if rc or not np.array_equal(ids[:n], want_ids(d, q)) or not (ids[n:] == GUARD).all():
                    errors.append((t, call, rc, L.sha1chunk_last_error()))
                    return
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((t, repr(e)))

    with pkg.DigestIndex(table) as ix:
        threads = [threading.Thread(target=worker, args=(t, ix)) for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    assert not errors, errors[:3]


# ------------------------------------------------------------- 8. refusals --
def _second_device(pkg):
    if pkg.device_count() < 2:
        pytest.skip("one device: no index of another device")
    pkg.set_device(1)


# row -> (set-up, expected code, arguments (ix, digests, n, ids) -> backend call)
BACKEND_REFUSALS = {
    "lookup_device: digests at 2 mod 4": (None, EALIGN, lambda be, a: be.s1be_index_lookup_device_async(
        a.ix, a.d_dig + 2, a.n, a.d_ids, None)),
    "lookup_device: ids at 1 mod 4": (None, EALIGN, lambda be, a: be.s1be_index_lookup_device_async(
        a.ix, a.d_dig, a.n, a.d_ids + 1, None)),
    "lookup_device: n = 2^32 - 255": (None, EINVAL, lambda be, a: be.s1be_index_lookup_device_async(
        a.ix, a.d_dig, 2 ** 32 - 255, a.d_ids, None)),
    "lookup: n = 2^32 - 255": (None, EINVAL, lambda be, a: be.s1be_index_lookup(a.ix, a.h_dig, 2 ** 32 - 255, a.h_ids)),
    "lookup: ids at 2 mod 4": (None, EALIGN, lambda be, a: be.s1be_index_lookup(a.ix, a.h_dig, a.n, a.h_ids + 2)),
    "lookup: null index": (None, EINVAL, lambda be, a: be.s1be_index_lookup(None, a.h_dig, a.n, a.h_ids)),
    "match_batch: n = 2^32 - 1024": (None, EINVAL, lambda be, a: be.s1be_match_batch(
        a.ix, a.h_dig, a.h_off, a.h_len, 2 ** 32 - 1024, a.h_ids, HOST)),
    "match_batch: ALL_DEVICES": (None, EINVAL, lambda be, a: be.s1be_match_batch(
        a.ix, a.h_dig, a.h_off, a.h_len, 2, a.h_ids, 2)),
    "lookup_device: index of another device": (_second_device, EINVAL, lambda be, a: a.L.sha1chunk_index_lookup_device_async(
        a.ix, a.d_dig, a.n, a.d_ids, None)),
    "lookup: index of another device": (_second_device, EINVAL, lambda be, a: a.L.sha1chunk_index_lookup(
        a.ix, a.h_dig, a.n, a.h_ids)),
    "match_batch: index of another device": (_second_device, EINVAL, lambda be, a: a.L.sha1chunk_match_batch(
        a.ix, a.h_dig, a.h_off, a.h_len, 2, a.h_ids, HOST)),
}


@pytest.mark.parametrize("row", list(BACKEND_REFUSALS))
def test_backend_refusals(pkg, dev, backend, row):
    """Each refusal leaves the outputs alone and is followed by a valid call."""
    torch = dev
    setup, code, call = BACKEND_REFUSALS[row]
    rng = np.random.default_rng(9)
    table = digests(rng, 40)

    class A:
        pass
    a = A()
    a.L, a.n = pkg.lib(), 40
    queries = np.ascontiguousarray(table[::-1])
    h_ids = np.full(a.n + TAIL, GUARD, np.uint32)
    d_dig = torch.from_numpy(queries).cuda()
    d_ids = torch.from_numpy(np.full(a.n + TAIL, GUARD, np.uint32).view(np.int32)).cuda()
    off, ln = np.array([0, 20], np.uint64), np.array([20, 20], np.uint32)
    a.h_dig, a.h_ids, a.d_dig, a.d_ids = queries.ctypes.data, h_ids.ctypes.data, d_dig.data_ptr(), d_ids.data_ptr()
    a.h_off, a.h_len = off.ctypes.data, ln.ctypes.data
    with pkg.DigestIndex(table) as ix:
        a.ix = ix._ix
        try:
            if setup:
                setup(pkg)
            assert call(backend, a) == code, (backend.s1be_last_error(), a.L.sha1chunk_last_error())
            torch.cuda.synchronize()
            assert (h_ids == GUARD).all() and (d_ids.cpu().numpy().view(np.uint32) == GUARD).all()
        finally:
            pkg.set_device(0)
        assert np.array_equal(host_lookup(pkg, ix, queries), np.arange(39, -1, -1))
        assert np.array_equal(device_lookup(pkg, torch, ix, queries), np.arange(39, -1, -1))
