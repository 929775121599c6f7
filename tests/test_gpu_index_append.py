"""GPU: growing the digest index (include/sha1chunk.h, "Digest index":
sha1chunk_index_reserve / _capacity / _append_device_async / _append and
sha1chunk_admit_batch; csrc/sha1_index.hip, rt_index.hip).  Exact: every
answer against a Python dict of the lowest ADMITTED position (a skipped digest
uses its position up and answers NO_MATCH), guard words behind every id
array.  The helpers are those of tests/test_gpu_index.py."""
import ctypes as C
import threading

import numpy as np
import pytest

import stream_gate as sg
from test_gpu_index import (CHAIN_SEED, DEVICE, EALIGN, EINVAL, GUARD, HOST, NO_MATCH, TAIL, _second_device,  # noqa: F401
                            _splitmix64, backend, dev, dev_off16, device_lookup, digests, host_lookup, index_stats,
                            off16, want_ids)

pytestmark = pytest.mark.gpu


def slots_for(m):
    return max(8, 1 << (2 * m - 1).bit_length()) if m else 8


@pytest.fixture(scope="module")
def be(backend):
    """The backend's own entry points of the appends, and its append counters."""
    backend.s1be_index_append_stats.restype = C.c_int
    backend.s1be_index_append_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    backend.s1be_index_reserve.argtypes = [C.c_void_p, C.c_size_t]
    backend.s1be_index_append.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    backend.s1be_index_append_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    backend.s1be_admit_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.c_void_p, C.c_uint]
    return backend


def append_stats(be, ix):
    """[longest append probe where one left its home, appended entries whose
    digest was in place, appended entries whose probe wrapped]."""
    out = (C.c_uint64 * 3)()
    assert be.s1be_index_append_stats(ix._ix, out) == 0, be.s1be_last_error()
    return list(out)


class Model:
    """What the index must answer: digest bytes -> lowest admitted position."""

    def __init__(self, table):
        self.low, self.size, self.given = {}, 0, [np.zeros((0, 20), np.uint8)]
        self.append(table, None)

    def append(self, rows, skip):
        for i, row in enumerate(rows):
            if skip is None or not skip[i]:
                self.low.setdefault(row.tobytes(), self.size + i)
        self.size += rows.shape[0]
        self.given.append(rows)

    def queries(self, rng, misses=40):
        q = np.concatenate(self.given + [digests(rng, misses)])
        return q[rng.permutation(q.shape[0])]


def odd_bytes(torch, values):
    """Bytes on the device at an address that is 1 mod 4 -> (tensor, address)."""
    t = torch.zeros(values.size + 8, dtype=torch.uint8, device="cuda")
    at = (1 - t.data_ptr()) % 4
    t[at:at + values.size] = torch.from_numpy(np.ascontiguousarray(values, np.uint8)).cuda()
    return t, t.data_ptr() + at


def raw_append(pkg, torch, ix, rows, skip, form):
    """One append through the C ABI -> its return code.  Digests 4 mod 16, skip
    bytes 1 mod 4; the device form on the current stream, then a synchronise."""
    k = rows.shape[0]
    L = pkg.lib()
    if form == "host":
        q = off16(rows)
        sk = None
        if skip is not None:
            buf = np.zeros(k + 8, np.uint8)
            at = (1 - buf.ctypes.data) % 4
            buf[at:at + k] = skip
            sk = buf.ctypes.data + at
        return L.sha1chunk_index_append(ix._ix, q.ctypes.data, k, sk)
    keep, addr = dev_off16(torch, rows)
    keep2, sk = (None, None) if skip is None else odd_bytes(torch, skip)
    rc = L.sha1chunk_index_append_device_async(ix._ix, addr, k, sk, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def check_answers(pkg, torch, ix, model, rng, device=None):
    q = model.queries(rng)
    want = want_ids(model.low, q)
    assert ix.size == model.size
    if device is not False:
        assert np.array_equal(device_lookup(pkg, torch, ix, q), want)
    if device is not True:
        assert np.array_equal(host_lookup(pkg, ix, q), want)


def call_rows(rng, model, k):
    """k digests: a tenth repeat earlier ones (admitted or skipped), a few
    repeat digests of the same call."""
    rows = digests(rng, k)
    earlier = np.concatenate(model.given)
    if earlier.shape[0]:
        rep = rng.choice(k, max(1, k // 10), replace=False) if k > 1 else np.zeros(0, int)
        rows[rep] = earlier[rng.integers(0, earlier.shape[0], rep.size)]
    if k >= 63:
        dst = rng.choice(k, 4, replace=False)
        rows[dst[:2]] = rows[dst[2:]]
    return rows


# ----------------------------------------- 1. a sequence against a dict -------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("m", [0, 1, 1000])
def test_sequence_against_a_dict(pkg, dev, backend, m, form):
    torch = dev
    rng = np.random.default_rng(1000 + m)
    table = digests(rng, m)
    model = Model(table)
    with pkg.DigestIndex(table) as ix:
        assert (ix.size, ix.capacity) == (m, m)
        assert index_stats(backend, ix)[0] == slots_for(m)
        ix.reserve(20000)
        assert (ix.size, ix.capacity) == (m, 20000)
        assert index_stats(backend, ix)[0] == slots_for(20000) == 65536
        check_answers(pkg, torch, ix, model, rng)
        for k in (1, 63, 64, 65, 257, 5000):
            rows = call_rows(rng, model, k)
            skip = (rng.integers(0, 4, k) == 0) * rng.integers(1, 256, k)  # a quarter skipped, any non-zero byte
            skip = skip.astype(np.uint8)
            assert raw_append(pkg, torch, ix, rows, skip, form) == 0, pkg.lib().sha1chunk_last_error()
            model.append(rows, skip)
            assert (ix.size, ix.capacity) == (model.size, 20000)
            check_answers(pkg, torch, ix, model, rng, device=(k % 2 == 1))
        # no skip array: every digest admitted
        rows = call_rows(rng, model, 100)
        assert raw_append(pkg, torch, ix, rows, None, form) == 0
        model.append(rows, None)
        check_answers(pkg, torch, ix, model, rng)


# ----------------------------------------------------------------- 2. growth --
def test_growth_by_the_host_append(pkg, dev, backend):
    torch = dev
    rng = np.random.default_rng(2)
    table = digests(rng, 3)
    model = Model(table)
    with pkg.DigestIndex(table) as ix:
        assert index_stats(backend, ix)[0] == 8 and ix.capacity == 3
        never = digests(rng, 1)  # skipped before the first growth, admitted nowhere
        assert ix.append(never, skip=[1]) == 3
        model.append(never, [1])
        model.given.pop()  # never repeated by a later call, and asked for on its own below
        assert ix.capacity >= 6 and ix.lookup(never)[0] == NO_MATCH
        growths = 1
        for k in (1, 2, 5, 20, 100, 1000, 10000, 70000 - 11132):
            cap = ix.capacity
            rows = call_rows(rng, model, k)
            skip = (rng.integers(0, 5, k) == 0).astype(np.uint8)
            first = ix.append(rows, skip)
            assert first == model.size
            model.append(rows, skip)
            if model.size > cap:
                growths += 1
                assert ix.capacity >= max(2 * cap, model.size)  # at least doubled
            else:
                assert ix.capacity == cap
            assert ix.capacity <= 2 ** 31 and ix.size == model.size
            assert index_stats(backend, ix)[0] == slots_for(ix.capacity)
            check_answers(pkg, torch, ix, model, rng, device=(k % 2 == 0))  # every earlier answer unchanged
            assert ix.lookup(never)[0] == NO_MATCH
        assert model.size == 70000 and growths >= 6
        before = (ix.size, ix.capacity, index_stats(backend, ix))
        ix.reserve(ix.capacity - 1)
        ix.reserve(0)
        assert (ix.size, ix.capacity, index_stats(backend, ix)) == before
        ix.reserve(ix.capacity + 1)
        assert ix.capacity == before[1] + 1 and index_stats(backend, ix)[0] == slots_for(before[1] + 1)
        check_answers(pkg, torch, ix, model, rng)
        # admitted at last, the digest answers the later position
        assert ix.append(never) == 70000 and ix.lookup(never)[0] == 70000


# ----------------------------------------------------------------- 3. chains --
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("again", [False, True])
def test_chains_appended_into_a_table(pkg, dev, be, form, again):
    """200 digests of one home in four calls of 50, behind 1000 random digests;
    `again`: a duplicate of each in a later call, the lowest position wins."""
    torch = dev
    rng = np.random.default_rng(3)
    table = digests(rng, 1000)
    model = Model(table)
    chain = digests(rng, 200)
    chain[:, :8] = np.frombuffer(_splitmix64(CHAIN_SEED + 1).to_bytes(8, "little"), np.uint8)
    assert len({r.tobytes() for r in chain}) == 200
    with pkg.DigestIndex(table) as ix:
        ix.reserve(1400)
        calls = [chain[50 * c:50 * c + 50] for c in range(4)]
        if again:
            calls += [chain[::-1][50 * c:50 * c + 50] for c in range(4)]
        for rows in calls:
            assert raw_append(pkg, torch, ix, rows, None, form) == 0, pkg.lib().sha1chunk_last_error()
            model.append(rows, None)
            check_answers(pkg, torch, ix, model, rng)
        assert np.array_equal(ix.lookup(chain), 1000 + np.arange(200))
        same_home = chain.copy()
        same_home[:, 8:] ^= 0x55
        assert (ix.lookup(same_home) == NO_MATCH).all()
        st = append_stats(be, ix)
        # the link that arrived last passed the 199 others
        assert st[0] >= 200 and st[1] == (200 if again else 0), st
        assert ix.size == (1400 if again else 1200)


# ------------------------------------------------------------------- 4. skip --
@pytest.mark.parametrize("form", ["host", "device"])
def test_skip(pkg, dev, backend, form):
    torch = dev
    rng = np.random.default_rng(4)
    table = digests(rng, 10)
    a, b = digests(rng, 1), digests(rng, 1)
    with pkg.DigestIndex(table) as ix:
        ix.reserve(64)

        def app(rows, skip):
            assert raw_append(pkg, torch, ix, rows, None if skip is None else np.array(skip, np.uint8), form) == 0

        def answers():
            q = np.concatenate([table, a, b, digests(np.random.default_rng(44), 10)])
            return np.concatenate([host_lookup(pkg, ix, q), device_lookup(pkg, torch, ix, q)])

        app(a, [0x80])                            # position 10, not admitted
        assert ix.size == 11 and ix.lookup(a)[0] == NO_MATCH
        app(np.concatenate([b, a]), [0, 0])       # positions 11 and 12
        assert ix.lookup(np.concatenate([a, b])).tolist() == [12, 11]
        app(np.concatenate([a, table[3:4], b]), [1, 1, 1])  # skipped duplicates of admitted digests
        assert ix.lookup(np.concatenate([a, table[3:4], b])).tolist() == [12, 3, 11]
        before, size = answers(), ix.size
        app(digests(rng, 20), [1] * 20)           # an all-skipped call uses 20 positions up
        assert ix.size == size + 20 and np.array_equal(answers(), before)
        app(np.zeros((0, 20), np.uint8), None)    # k == 0
        app(np.zeros((0, 20), np.uint8), [])
        assert ix.size == size + 20 and np.array_equal(answers(), before)
        assert pkg.lib().sha1chunk_index_append(ix._ix, None, 0, None) == 0
        assert pkg.lib().sha1chunk_index_append_device_async(ix._ix, None, 0, None, None) == 0
        assert ix.size == size + 20 and ix.capacity == 64


# --------------------------------- 5. the device form refuses, never allocates --
def test_device_form_refuses_when_capacity_is_short(pkg, dev, backend):
    torch = dev
    rng = np.random.default_rng(5)
    table = digests(rng, 100)
    model = Model(table)
    rows = digests(rng, 29)
    with pkg.DigestIndex(table) as ix:
        ix.reserve(128)
        stats = index_stats(backend, ix)
        assert raw_append(pkg, torch, ix, rows, None, "device") == EINVAL  # 100 + 29 = 128 + 1
        assert b"sha1chunk_index_reserve" in pkg.lib().sha1chunk_last_error()
        with pytest.raises(pkg.Sha1ChunkError) as ei:
            ix.append_device(torch.from_numpy(rows).cuda())
        assert ei.value.code == EINVAL
        assert (ix.size, ix.capacity) == (100, 128) and index_stats(backend, ix) == stats
        check_answers(pkg, torch, ix, model, rng)
        assert (ix.lookup(rows) == NO_MATCH).all()
        # one fewer fits exactly
        assert raw_append(pkg, torch, ix, rows[:28], None, "device") == 0
        model.append(rows[:28], None)
        assert (ix.size, ix.capacity) == (128, 128)
        check_answers(pkg, torch, ix, model, rng)
        assert raw_append(pkg, torch, ix, rows[28:], None, "device") == EINVAL
        ix.reserve(129)
        assert raw_append(pkg, torch, ix, rows[28:], None, "device") == 0
        model.append(rows[28:], None)
        assert (ix.size, ix.capacity) == (129, 129)
        check_answers(pkg, torch, ix, model, rng)


# ------------------------- 6. the receive path: one stream, one synchronise ----
def test_receive_path_on_one_stream(pkg, dev, oracle):
    torch = dev
    rng = np.random.default_rng(6)
    n, L, m = 256, 4096, 500
    host = oracle.synth_chunks(0, n, L)
    off, lens = np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32)
    dig = oracle.hash_batch(host, off, lens)
    bad = np.arange(n) % 5 == 4
    expected = dig.copy()
    expected[bad, rng.integers(0, 20, int(bad.sum()))] ^= 0x04
    table = digests(rng, m)
    want = np.where(bad, NO_MATCH, m + np.arange(n)).astype(np.uint32)
    s = torch.cuda.Stream()
    with pkg.DigestIndex(table) as ix, torch.cuda.stream(s):
        ix.reserve(m + n)
        buf = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        d_dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
        d_exp = torch.from_numpy(expected).cuda()
        mis = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        ids = torch.from_numpy(np.full(n + TAIL, GUARD, np.uint32).view(np.int32)).cuda()
        ids2 = torch.from_numpy(np.full(n + TAIL, GUARD, np.uint32).view(np.int32)).cuda()
        s.synchronize()
        pkg.synth_fill_device(buf, 0, n, L, stream=s)
        pkg.hash_uniform_device(buf, L, n, d_dig, stream=s)
        pkg.sha1chunk.compare_device(d_dig, d_exp, mis, stream=s)
        assert ix.append_device(d_dig, n, skip=mis, stream=s) == m
        ix.lookup_device(d_exp, ids, n=n, stream=s)
        ix.lookup_device(d_dig, ids2, n=n, stream=s)
        assert ix.size == m + n  # known at enqueue
        s.synchronize()
        assert np.array_equal(mis.cpu().numpy(), bad.astype(np.uint8))
        got, got2 = ids.cpu().numpy().view(np.uint32), ids2.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:n], want) and (got[n:] == GUARD).all()
        # the true digest of a chunk that failed was skipped, not admitted
        assert np.array_equal(got2[:n], want) and (got2[n:] == GUARD).all()
        probe = np.concatenate([table, dig, expected])
        reference = ix.lookup(probe)
    # admit_batch, host and device forms: the same verdicts, the same set
    with pkg.DigestIndex(table) as ix:
        assert np.array_equal(ix.admit_batch(host, off, lens, expected), bad.astype(np.uint8))
        assert ix.size == m + n and ix.capacity >= m + n
        assert np.array_equal(ix.lookup(probe), reference)
    with pkg.DigestIndex(table) as ix:
        args = (torch.from_numpy(host).cuda(), torch.from_numpy(off.view(np.int64)).cuda(),
                torch.from_numpy(lens.view(np.int32)).cuda(), torch.from_numpy(expected).cuda())
        mis = torch.full((n + TAIL,), 0xEE, dtype=torch.uint8, device="cuda")
        with pytest.raises(pkg.Sha1ChunkError) as ei:  # the device form never grows
            ix.admit_batch(*args, mis)
        assert ei.value.code == EINVAL and "sha1chunk_index_reserve" in str(ei.value)
        assert ix.size == m and (mis.cpu().numpy() == 0xEE).all()
        ix.reserve(m + n)
        ix.admit_batch(*args, mis)
        got = mis.cpu().numpy()
        assert np.array_equal(got[:n], bad.astype(np.uint8)) and (got[n:] == 0xEE).all()
        assert ix.size == m + n
        assert np.array_equal(ix.lookup(probe), reference)


# ------------------------------------------------------------ 7. stream order --
def test_append_then_lookup_behind_a_gated_stream(pkg, dev):
    """tests/test_gpu_stream_order.py's sequence around append -> lookup: gate,
    producer (true digests and skip bytes into the inputs), append, lookup of
    the same digests, consumer, clobber (the decoy).  Every row differs between
    the instances: a digest is skipped in exactly one of them."""
    torch = dev
    cx = sg.Context(pkg, torch, None)  # no case here uses the streaming trio
    gate = sg.Gate(pkg, torch)
    s = sg.independent_stream(torch, gate)
    rng = np.random.default_rng(7)
    m, k = 1000, 300
    table = digests(rng, m)
    inst = []
    for which in (0, 1):
        rows = digests(rng, k)
        skip = ((np.arange(k) % 3 == 0) ^ bool(which)).astype(np.uint8)
        ids = np.where(skip != 0, NO_MATCH, m + np.arange(k)).astype(np.uint32)
        inst.append((rows, skip, sg.rows(ids, 4)))
    c = sg.Case(cx, "append -> lookup")
    d_rows = c.add_in("digests", inst[0][0], inst[1][0])
    d_skip = c.add_in("skip", inst[0][1], inst[1][1])
    d_ids = c.add_out("ids", inst[0][2], inst[1][2], dtype="int32")
    warm, ix = pkg.DigestIndex(table), pkg.DigestIndex(table)
    with warm, ix:
        warm.reserve(m + k)
        ix.reserve(m + k)
        target = [warm]

        def call(st):
            assert target[0].append_device(d_rows, k, skip=d_skip, stream=st) == m
            target[0].lookup_device(d_rows, d_ids, n=k, stream=st)
        c.call = call
        c.check_instances()
        sg.warm_up(c, s, s)
        target[0] = ix
        with torch.cuda.stream(s):
            gated = sg.enqueue(c, s, gate)
        s.synchronize()
        gate.check()
        c.check("behind the gate")
        sg.returned_while_gated(c, gated)
        assert ix.size == m + k
        assert np.array_equal(ix.lookup(inst[0][0]), inst[0][2].view(np.uint32).reshape(-1))
        assert (ix.lookup(inst[1][0]) == NO_MATCH).all()


# ---------------------------------------------------------------- 8. threads --
def test_host_append_beside_host_lookups(pkg, dev):
    rng = np.random.default_rng(8)
    m, calls, per = 100, 64, 100
    table = digests(rng, m)
    new = digests(rng, calls * per)
    everything = np.concatenate([table, new])
    assert len({r.tobytes() for r in everything}) == everything.shape[0]
    L = pkg.lib()
    errors = []
    done = threading.Event()

    def appender(ix):
        try:
            for j in range(calls):
                rows = np.ascontiguousarray(new[per * j:per * (j + 1)])
                if L.sha1chunk_index_append(ix._ix, rows.ctypes.data, per, None):
                    errors.append(("append", j, L.sha1chunk_last_error()))
                    return
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(("append", repr(e)))
        finally:
            done.set()

    def reader(t, ix):
        r = np.random.default_rng(80 + t)
        seen = np.zeros(everything.shape[0], bool)
        seen[:m] = True
        try:
            last, rounds = False, 0
            while not last:
                rounds += 1
                last = rounds >= 200 and done.is_set()  # and one more round after the appender has finished
                n = int(r.integers(1, 400))
                pick = r.integers(0, everything.shape[0], n)
                q = np.ascontiguousarray(everything[pick])
                ids = np.full(n + TAIL, GUARD, np.uint32)
                rc = L.sha1chunk_index_lookup(ix._ix, q.ctypes.data, n, ids.ctypes.data)
                got = ids[:n]
                found = got == pick
                ok = rc == 0 and (found | (got == NO_MATCH)).all() and (ids[n:] == GUARD).all()
                if not ok or (seen[pick] & ~found).any():  # once seen, never NO_MATCH again
                    errors.append((t, rc, L.sha1chunk_last_error(), pick[~found][:5].tolist(), got[~found][:5].tolist()))
                    return
                seen[pick[found]] = True
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    with pkg.DigestIndex(table) as ix:
        threads = [threading.Thread(target=appender, args=(ix,))] + \
                  [threading.Thread(target=reader, args=(t, ix)) for t in range(3)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors[:3]
        assert ix.size == m + calls * per and ix.capacity >= ix.size
        assert np.array_equal(ix.lookup(everything), np.arange(everything.shape[0]))


# ------------------------------------------------------ 9. backend refusals ----
# row -> (set-up, expected code, arguments -> backend call): what the front
# end's checks never let through, and an index of another device
APPEND_REFUSALS = {
    "append_device: digests at 2 mod 4": (None, EALIGN, lambda be, a: be.s1be_index_append_device_async(
        a.ix, a.d_dig + 2, a.k, a.d_skip, None)),
    "append: digests at 1 mod 4": (None, EALIGN, lambda be, a: be.s1be_index_append(a.ix, a.h_dig + 1, a.k, a.h_skip)),
    "append_device: k = 2^32 - 255": (None, EINVAL, lambda be, a: be.s1be_index_append_device_async(
        a.ix, a.d_dig, 2 ** 32 - 255, a.d_skip, None)),
    "append: k = 2^32 - 255": (None, EINVAL, lambda be, a: be.s1be_index_append(a.ix, a.h_dig, 2 ** 32 - 255, a.h_skip)),
    "append_device: size + k = 2^31 + 1": (None, EINVAL, lambda be, a: be.s1be_index_append_device_async(
        a.ix, a.d_dig, 2 ** 31 - 39, a.d_skip, None)),
    "append: size + k = 2^31 + 1": (None, EINVAL, lambda be, a: a.L.sha1chunk_index_append(
        a.ix, a.h_dig, 2 ** 31 - 39, a.h_skip)),
    "append: null index": (None, EINVAL, lambda be, a: be.s1be_index_append(None, a.h_dig, a.k, a.h_skip)),
    "append: null digests": (None, EINVAL, lambda be, a: be.s1be_index_append(a.ix, None, a.k, a.h_skip)),
    "reserve: 2^31 + 1": (None, EINVAL, lambda be, a: be.s1be_index_reserve(a.ix, 2 ** 31 + 1)),
    "admit_batch: n = 2^32 - 1024": (None, EINVAL, lambda be, a: be.s1be_admit_batch(
        a.ix, a.h_dig, a.h_off, a.h_len, 2 ** 32 - 1024, a.h_dig, a.h_mis, HOST)),
    "admit_batch: ALL_DEVICES": (None, EINVAL, lambda be, a: be.s1be_admit_batch(
        a.ix, a.h_dig, a.h_off, a.h_len, 2, a.h_dig, a.h_mis, 2)),
    "admit_batch: size + n = 2^31 + 1": (None, EINVAL, lambda be, a: a.L.sha1chunk_admit_batch(
        a.ix, a.h_dig, a.h_off, a.h_len, 2 ** 31 - 39, a.h_dig, a.h_mis, HOST)),
    "append_device: index of another device": (_second_device, EINVAL, lambda be, a: a.L.sha1chunk_index_append_device_async(
        a.ix, a.d_dig, a.k, a.d_skip, None)),
    "append: index of another device": (_second_device, EINVAL, lambda be, a: a.L.sha1chunk_index_append(
        a.ix, a.h_dig, a.k, a.h_skip)),
    "reserve: index of another device": (_second_device, EINVAL, lambda be, a: a.L.sha1chunk_index_reserve(a.ix, 1000)),
    "admit_batch: index of another device": (_second_device, EINVAL, lambda be, a: a.L.sha1chunk_admit_batch(
        a.ix, a.h_dig, a.h_off, a.h_len, 2, a.h_dig, a.h_mis, HOST)),
}


@pytest.mark.parametrize("row", list(APPEND_REFUSALS))
def test_backend_refusals(pkg, dev, be, row):
    """Each refusal leaves the index and the outputs alone and is followed by a
    valid call."""
    torch = dev
    setup, code, call = APPEND_REFUSALS[row]
    rng = np.random.default_rng(9)
    table = digests(rng, 40)
    rows = digests(rng, 8)

    class A:
        pass
    a = A()
    a.L, a.k = pkg.lib(), 8
    h_rows = np.ascontiguousarray(np.concatenate([rows, np.zeros((1, 20), np.uint8)]))  # room for a shifted address
    h_skip, h_mis = np.zeros(8, np.uint8), np.full(8 + TAIL, 0xA5, np.uint8)
    d_rows, d_skip = torch.from_numpy(h_rows).cuda(), torch.zeros(8, dtype=torch.uint8, device="cuda")
    off, ln = np.array([0, 20], np.uint64), np.array([20, 20], np.uint32)
    a.h_dig, a.h_skip, a.h_mis = h_rows.ctypes.data, h_skip.ctypes.data, h_mis.ctypes.data
    a.d_dig, a.d_skip, a.h_off, a.h_len = d_rows.data_ptr(), d_skip.data_ptr(), off.ctypes.data, ln.ctypes.data
    with pkg.DigestIndex(table) as ix:
        ix.reserve(64)
        a.ix = ix._ix
        stats = index_stats(be, ix)
        try:
            if setup:
                setup(pkg)
            assert call(be, a) == code, (be.s1be_last_error(), a.L.sha1chunk_last_error())
            torch.cuda.synchronize()
            assert (h_mis == 0xA5).all()
        finally:
            pkg.set_device(0)
        assert (ix.size, ix.capacity) == (40, 64) and index_stats(be, ix) == stats
        q = np.concatenate([table[::-1], rows])
        want = np.concatenate([np.arange(39, -1, -1), np.full(8, NO_MATCH)]).astype(np.uint32)
        assert np.array_equal(host_lookup(pkg, ix, q), want)
        assert raw_append(pkg, torch, ix, rows, None, "device") == 0
        want[40:] = 40 + np.arange(8)
        assert np.array_equal(device_lookup(pkg, torch, ix, q), want)
