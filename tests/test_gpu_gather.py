"""GPU: messages given as segment lists (include/sha1chunk.h, "Messages given
as segment lists"; csrc/sha1_gather.hip, rt_gather.hip).  Bit-exact: the
reassembled bytes against a numpy model with 0xA5 guards, the digests against
hashlib."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import reassembly_replay as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5
SKIPPED = 0xFFFFFFFF
EINVAL = -1
HOST, DEVICE, ALL_DEVICES = 0, 1, 2
CHUNK, BODY, NPACK, SLOT, HEADER = rr.CHUNK_LEN, rr.BODY, rr.NPACK, 1500, 16
EMPTY_DIGEST = "da39a3ee5e6b4b0d3255bfef95601890afd80709"


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert pkg.device_count() >= 1, pkg.lib().sha1chunk_last_error()
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


@pytest.fixture(scope="module")
def stats(pkg):
    """s1be_gather_stats: [sub-batches, gather launches, messages skipped,
    calls from device / pinned / pageable memory]."""
    pkg.lib()
    be = C.CDLL(os.path.join(os.path.dirname(pkg.sha1chunk.LIB_PATH), "libsha1chunk_hip.so"))
    be.s1be_gather_stats.restype = None
    be.s1be_gather_stats.argtypes = [C.POINTER(C.c_uint64), C.c_int]

    def read(reset=False):
        out = (C.c_uint64 * 6)()
        be.s1be_gather_stats(out, int(reset))
        return list(out)
    return read


def payload(rng, n):
    """n random bytes, none of them the guard value."""
    b = rng.integers(0, 255, n, dtype=np.uint8)
    b[b >= GUARD] += 1
    return b


def to_dev(torch, a):
    """A numpy array on the device (unsigned types as their signed twins)."""
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    a = a if a.flags.writeable else a.copy()
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


def sha1s(messages):
    return np.array([np.frombuffer(hashlib.sha1(m).digest(), np.uint8) for m in messages]).reshape(-1, 20)


def gather_on_device(pkg, torch, base, csr, dst_np, dst_off):
    """sha1chunk_gather_device_async into a copy of dst_np; (bytes, lengths)."""
    off, ln, first = csr
    dst = to_dev(torch, dst_np)
    out_len = torch.full((first.size - 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pkg.sha1chunk.gather_device(base, to_dev(torch, off), to_dev(torch, ln), to_dev(torch, first), dst,
                                to_dev(torch, np.asarray(dst_off, np.uint64)), out_lengths=out_len, n_segments=ln.size)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), out_len.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------- 1. seams ----
SEAM_LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1483, 1484, 1485]


def test_seams_and_alignment(pkg, dev):
    """Every (segment length, source start mod 16, destination start mod 16)
    as the first segment of a message of 2-3 segments, in one call, the
    messages in shuffled order, guards everywhere."""
    torch = dev
    rng = np.random.default_rng(1)
    msgs = []  # (dst alignment, [(src alignment, length), ...])
    k = 0
    for L in SEAM_LENGTHS:
        for sa in range(16):
            for da in range(16):
                rest = [(int(rng.integers(16)), SEAM_LENGTHS[(k + 5 * j) % len(SEAM_LENGTHS)]) for j in range(1, 2 + k % 2)]
                msgs.append((da, [(sa, L)] + rest))
                k += 1
    src_parts, segs, cur = [], [], 0
    for _, parts in msgs:
        for sa, L in parts:
            pad = (-cur) % 16 + sa + 32
            src_parts += [np.full(pad, GUARD, np.uint8), payload(rng, L)]
            segs.append((cur + pad, L))
            cur += pad + L
    src = np.concatenate(src_parts + [np.full(64, GUARD, np.uint8)])
    want_parts, dst_off, lengths, cur, s = [], [], [], 0, 0
    for da, parts in msgs:
        body = np.concatenate([src[o:o + L] for o, L in segs[s:s + len(parts)]])
        s += len(parts)
        pad = (-cur) % 16 + da + 16
        want_parts += [np.full(pad, GUARD, np.uint8), body]
        dst_off.append(cur + pad)
        lengths.append(body.size)
        cur += pad + body.size
    want = np.concatenate(want_parts + [np.full(48, GUARD, np.uint8)])
    # the call lists the messages in another order than they lie in
    order = rng.permutation(len(msgs))
    starts = np.cumsum([0] + [len(p) for _, p in msgs])
    lists = [[segs[j] for j in range(starts[i], starts[i + 1])] for i in order]
    csr = pkg.sha1chunk.segment_csr(lists)
    got, out_len = gather_on_device(pkg, torch, to_dev(torch, src), csr, np.full(want.size, GUARD, np.uint8),
                                    np.array(dst_off, np.uint64)[order])
    assert out_len.tolist() == [lengths[i] for i in order]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} wrong bytes, first at {bad[:8]}"
    # and the digests of the same call's messages
    dig = pkg.sha1chunk.hash_gather(to_dev(torch, src), csr)
    assert np.array_equal(dig, sha1s([want[dst_off[i]:dst_off[i] + lengths[i]].tobytes() for i in order]))


# ------------------------------------------------------ 2. packet shape ----
PACKET_N = (1, 2, 65, 130)


@pytest.fixture(scope="module")
def ring(pkg, dev):
    """130 chunks as 354 packets each in 1500-byte slots (16-byte header, then
    the payload), the slots of the whole ring permuted; on the host, on the
    device and in pinned memory."""
    torch = dev
    n = max(PACKET_N)
    rng = np.random.default_rng(2)
    chunks = np.frombuffer(rng.bytes(n * CHUNK), np.uint8).reshape(n, CHUNK)
    slot_of = rng.permutation(n * NPACK)
    host = np.full(n * NPACK * SLOT + 64, GUARD, np.uint8)
    lens = np.full(NPACK, BODY, np.uint32)
    lens[-1] = rr.LAST_BODY
    off = (slot_of.astype(np.uint64) * SLOT + HEADER).reshape(n, NPACK)
    for i in range(n):
        for k in range(NPACK):
            host[off[i, k]:off[i, k] + lens[k]] = chunks[i, BODY * k:BODY * k + lens[k]]
    pinned = pkg.sha1chunk.pinned_alloc(host.size)
    pinned[:] = host
    r = {"n": n, "chunks": chunks, "off": off, "lens": lens, "host": host, "device": to_dev(torch, host),
         "pinned": pinned, "digests": sha1s([c.tobytes() for c in chunks])}
    yield r
    torch.cuda.synchronize()
    pkg.sha1chunk.pinned_free(pinned)


def ring_csr(ring, n):
    return (np.ascontiguousarray(ring["off"][:n].reshape(-1)), np.tile(ring["lens"], n),
            np.arange(n + 1, dtype=np.uint32) * NPACK)


@pytest.mark.parametrize("n", PACKET_N)
@pytest.mark.parametrize("source", ["device", "pinned", "pageable"])
def test_packet_shape(pkg, dev, stats, ring, source, n):
    torch = dev
    csr = ring_csr(ring, n)
    base = {"device": ring["device"], "pinned": ring["pinned"], "pageable": ring["host"]}[source]
    want = ring["digests"][:n]
    if source != "pageable":  # the reassembled bytes (the device form reads device or pinned memory)
        stride = CHUNK + 128
        got, out_len = gather_on_device(pkg, torch, base, csr, np.full(n * stride + 64, GUARD, np.uint8),
                                        64 + np.arange(n, dtype=np.uint64) * stride)
        model = np.full(n * stride + 64, GUARD, np.uint8)
        for i in range(n):
            model[64 + i * stride:64 + i * stride + CHUNK] = ring["chunks"][i]
        assert (out_len == CHUNK).all()
        assert np.array_equal(got, model)
    stats(reset=True)
    assert np.array_equal(pkg.sha1chunk.hash_gather(base, csr), want)
    # every third expected digest corrupted, and one flipped bit in one payload
    exp = want.copy()
    exp[::3, 7] ^= 0x10
    flip_msg = n // 2
    where = int(ring["off"][flip_msg, 200]) + 700
    base[where] ^= 0x04
    try:
        if source == "device":
            torch.cuda.synchronize()
        mis = pkg.sha1chunk.verify_gather(base, csr, exp)
    finally:
        base[where] ^= 0x04
    want_mis = np.zeros(n, np.uint8)
    want_mis[::3] = 1
    want_mis[flip_msg] = 1
    assert mis.tolist() == want_mis.tolist()
    s = stats()
    print("gather_stats", source, n, s)
    assert s[0] == 2 and s[2] == 0
    assert s[3:] == {"device": [2, 0, 0], "pinned": [0, 2, 0], "pageable": [0, 0, 2]}[source]
    assert s[1] == (0 if source == "pageable" else 2)  # the pageable path runs no gather kernel


# ------------------------------------------- 3. shapes that break tiling ----
def test_shapes_that_break_tiling(pkg, dev):
    torch = dev
    rng = np.random.default_rng(3)
    src = payload(rng, 700000)
    big = 300 * 1024 + 7
    tiny, cur = [], 310000
    for L in rng.integers(1, 8, 4000):
        tiny.append((cur, int(L)))
        cur += int(L) + int(rng.integers(0, 3))
    shared = [(650001, 1484), (3, 1484), (640007, 436)]
    lists = [
        [],                                  # no segments
        [(17, 0), (900, 0), (0, 0)],         # only zero-length segments
        [(5, big)],                          # one segment longer than a tile, and many tiles
        tiny,                                # 4000 segments of 1-7 bytes
        [(100001, 5), (200002, 1484), (9, 2)],  # 1491 bytes: not a multiple of 4
        shared,
        shared,                              # the same segments again
        [(123, 1)],
    ]
    bodies = [np.concatenate([src[o:o + L] for o, L in m] + [np.zeros(0, np.uint8)]) for m in lists]
    csr = pkg.sha1chunk.segment_csr(lists)
    dig = pkg.sha1chunk.hash_gather(to_dev(torch, src), csr)
    assert np.array_equal(dig, sha1s([b.tobytes() for b in bodies]))
    assert dig[0].tobytes().hex() == EMPTY_DIGEST and dig[1].tobytes().hex() == EMPTY_DIGEST
    assert np.array_equal(dig[5], dig[6])
    # the bytes, at odd destination starts, guards between
    dst_off, cur = [], 0
    for i, b in enumerate(bodies):
        cur += 16 + (7 * i + 3) % 16
        dst_off.append(cur)
        cur += b.size
    model = np.full(cur + 64, GUARD, np.uint8)
    for o, b in zip(dst_off, bodies):
        model[o:o + b.size] = b
    got, out_len = gather_on_device(pkg, torch, to_dev(torch, src), csr, np.full(model.size, GUARD, np.uint8), dst_off)
    assert out_len.tolist() == [b.size for b in bodies]
    assert np.array_equal(got, model)


# ------------------------------------------------ 4. several sub-batches ----
def test_several_sub_batches(pkg, dev, stats, monkeypatch):
    torch = dev
    rng = np.random.default_rng(4)
    lens = [int(x) for x in rng.integers(4096, 600 * 1024, 40)]
    lens[17] = (3 << 19) + 11  # 1.5 MiB: larger than the 1 MiB cap, a sub-batch of its own
    src = np.frombuffer(rng.bytes(sum(lens) + 4096), np.uint8)
    lists, bodies, cur = [], [], 1
    for L in lens:  # 2-4 pieces each
        cuts = sorted(set([0, L] + [int(c) for c in rng.integers(1, L, int(rng.integers(1, 4)))]))
        pieces = [(cur + a, b - a) for a, b in zip(cuts, cuts[1:])]
        lists.append(pieces)
        bodies.append(src[cur:cur + L].tobytes())
        cur += L
    want = sha1s(bodies)
    # the sub-batches of the documented rule: whole messages, each on a 128-byte
    # line, packed size at most the cap, at least one message
    expect, packed = 1, 0
    for L in lens:
        b = (L + 127) // 128 * 128
        if packed and packed + b > 1 << 20:
            expect, packed = expect + 1, 0
        packed += b
    assert expect > 10
    monkeypatch.setenv("SHA1CHUNK_GATHER_STAGE_MIB", "1")
    for source, base in (("device", to_dev(torch, src)), ("pageable", src)):
        stats(reset=True)
        assert np.array_equal(pkg.sha1chunk.hash_gather(base, lists), want), source
        s = stats()
        print("gather_stats", source, s)
        assert s[0] == expect and s[1] == (expect if source == "device" else 0)
    monkeypatch.delenv("SHA1CHUNK_GATHER_STAGE_MIB")
    stats(reset=True)
    assert np.array_equal(pkg.sha1chunk.hash_gather(to_dev(torch, src), lists), want)
    assert stats()[0] == 1  # the default cap: one sub-batch


# -------------------------------------------------- 5. 64-bit offsets ----
def test_source_offsets_beyond_4gib(pkg, dev):
    torch = dev
    rng = np.random.default_rng(5)
    G = 1 << 32
    buf = torch.empty(G + (1 << 20), dtype=torch.uint8, device="cuda")
    # three written regions: near the start, a window around 2^32, the buffer's end
    regions = {1000: payload(rng, 1484), G - 8192: payload(rng, 16384), G + (1 << 20) - 1484: payload(rng, 1484)}
    for o, b in regions.items():
        buf[o:o + b.size] = torch.from_numpy(b).cuda()
    # below, across, above, ending at and starting at the boundary (segments may overlap)
    segs = [(1000, 1484), (G - 700, 1484), (G + 5000, 1484), (G - 3, 3), (G, 436), (G + (1 << 20) - 1484, 1484),
            (G - 1484, 1484)]

    def read(o, L):
        start = max(r for r in regions if r <= o)
        assert o + L <= start + regions[start].size
        return regions[start][o - start:o - start + L]
    data = {o: read(o, L) for o, L in segs}
    lists = [[segs[0], segs[1], segs[2]], [segs[3], segs[4]], [segs[5], segs[6], segs[1]]]
    bodies = [np.concatenate([data[o] for o, _ in m]) for m in lists]
    torch.cuda.synchronize()
    assert np.array_equal(pkg.sha1chunk.hash_gather(buf, lists), sha1s([b.tobytes() for b in bodies]))
    dst_off = [33, 33 + 5000, 33 + 10001]
    model = np.full(16384, GUARD, np.uint8)
    for o, b in zip(dst_off, bodies):
        model[o:o + b.size] = b
    got, out_len = gather_on_device(pkg, torch, buf, pkg.sha1chunk.segment_csr(lists),
                                    np.full(model.size, GUARD, np.uint8), dst_off)
    assert out_len.tolist() == [b.size for b in bodies]
    assert np.array_equal(got, model)


# ----------------------------------------------------------- 6. skips ----
def test_device_form_skips(pkg, dev, stats):
    """Each of the four skip conditions between valid neighbours: the
    neighbours are written, the skipped destinations are not, the length
    words say 0xFFFFFFFF."""
    torch = dev
    rng = np.random.default_rng(6)
    src = payload(rng, 8192)
    seg_off = np.array([0, 0, 100, 1700, 3000, 3100, 10, 20, 30, 5000, 6000, 6100], np.uint64)
    seg_len = np.array([9, 9, 1484, 37, 70, 1485, 0x7FFFFFFF, 0x7FFFFFFF, 1, 900, 64, 13], np.uint32)
    #            0 valid  1 reversed  2 valid  3 past the list  4 reversed  5 too long  6 no room  7 valid, to the end
    first = np.array([4, 6, 2, 4, 13, 6, 9, 10, 12], np.uint32)
    dst_bytes = 8000
    dst_off = np.array([35, 2000, 2101, 4000, 4100, 4200, 7101, dst_bytes - 77, ], np.uint64)
    bodies = {0: np.concatenate([src[3000:3070], src[3100:3100 + 1485]]),
              2: np.concatenate([src[100:100 + 1484], src[1700:1737]]),
              7: np.concatenate([src[6000:6064], src[6100:6113]])}
    assert bodies[7].size == 77 and int(dst_off[6]) + 900 == dst_bytes + 1
    model = np.full(dst_bytes + 256, GUARD, np.uint8)  # the tensor is longer than dst_bytes says
    for i, b in bodies.items():
        model[int(dst_off[i]):int(dst_off[i]) + b.size] = b
    stats(reset=True)
    dst = to_dev(torch, np.full(model.size, GUARD, np.uint8))
    out_len = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pkg.sha1chunk.gather_device(to_dev(torch, src), to_dev(torch, seg_off), to_dev(torch, seg_len),
                                to_dev(torch, first), dst, to_dev(torch, dst_off), out_lengths=out_len,
                                dst_bytes=dst_bytes)
    torch.cuda.synchronize()
    want_len = [bodies[0].size, SKIPPED, bodies[2].size, SKIPPED, SKIPPED, SKIPPED, SKIPPED, 77]
    assert out_len.cpu().numpy().view(np.uint32).tolist() == want_len
    assert np.array_equal(dst.cpu().numpy(), model)
    s = stats()
    assert s[1] == 1 and s[2] == 5, s
    # a NULL length array is allowed
    dst2 = to_dev(torch, np.full(model.size, GUARD, np.uint8))
    pkg.sha1chunk.gather_device(to_dev(torch, src), to_dev(torch, seg_off), to_dev(torch, seg_len),
                                to_dev(torch, first), dst2, to_dev(torch, dst_off), dst_bytes=dst_bytes)
    torch.cuda.synchronize()
    assert np.array_equal(dst2.cpu().numpy(), model)


def test_host_form_refusals_then_valid_calls(pkg, dev):
    """One table of refusals of the host-array forms on a device, outputs
    untouched, each followed by a valid call."""
    torch = dev
    L = pkg.lib()
    rng = np.random.default_rng(7)
    src = payload(rng, 4096)
    d_src = to_dev(torch, src)
    off = np.array([0, 10, 100, 7, 2000], np.uint64)
    ln = np.array([10, 90, 0, 3, 1484], np.uint32)
    first = np.array([0, 2, 2, 5], np.uint32)
    bodies = [np.concatenate([src[0:10], src[10:100]]), np.zeros(0, np.uint8), np.concatenate([src[7:10], src[2000:3484]])]
    want = sha1s([b.tobytes() for b in bodies])

    def call(verify=False, base=True, off_=True, ln_=None, n_segments=5, first_=first, n=3, out=True, flags=DEVICE):
        lens = ln if ln_ is None else np.array(ln_, np.uint32)
        fst = None if first_ is None else np.array(first_, np.uint32)
        dig = np.full(60, 0xAA, np.uint8)
        mis = np.full(3, 0xAA, np.uint8)
        b = (d_src.data_ptr() if flags & DEVICE else src.ctypes.data) if base else None
        head = (b, off.ctypes.data if off_ else None, lens.ctypes.data, n_segments,
                None if fst is None else fst.ctypes.data, n)
        if verify:
            rc = L.sha1chunk_verify_gather_batch(*head, want.ctypes.data, mis.ctypes.data if out else None, flags)
        else:
            rc = L.sha1chunk_hash_gather_batch(*head, dig.ctypes.data if out else None, flags)
        return rc, dig, mis

    rows = {
        "null base": dict(base=False),
        "null seg_offsets": dict(off_=False),
        "null seg_first": dict(first_=None),
        "null digests": dict(out=False),
        "null mismatch": dict(verify=True, out=False),
        "reversed range": dict(first_=(0, 3, 2, 5)),
        "range past the list": dict(first_=(0, 2, 2, 6)),
        "message of 2^32 - 1 bytes": dict(ln_=(0xFFFFFFFF, 0, 0, 0, 0)),
        "ALL_DEVICES": dict(flags=ALL_DEVICES),
        "DEVICE | ALL_DEVICES": dict(flags=DEVICE | ALL_DEVICES),
        "n = 2^32 - 1024": dict(n=2 ** 32 - 1024),
        "n_segments = 2^32 - 1024": dict(n_segments=2 ** 32 - 1024),
        "verify, reversed range, host": dict(verify=True, first_=(2, 0, 2, 5), flags=HOST),
    }
    for name, kw in rows.items():
        rc, dig, mis = call(**kw)
        assert rc == EINVAL, (name, rc, L.sha1chunk_last_error())
        assert L.sha1chunk_last_error() != b"", name
        assert (dig == 0xAA).all() and (mis == 0xAA).all(), name
        rc, dig, mis = call(flags=DEVICE if len(name) % 2 else HOST)
        assert rc == 0, (name, L.sha1chunk_last_error())
        assert np.array_equal(dig.reshape(3, 20), want), name
    rc, dig, mis = call(verify=True)
    assert rc == 0 and mis.tolist() == [0, 0, 0]


# ------------------------------------------ 7. reference arrival order ----
class Recorded:
    """The chunk's bytes; records which packets replay_attempt delivers, in
    order (it slices the body of every packet it accepts into the window)."""

    def __init__(self, data):
        self.data, self.seqs = data, []

    def __len__(self):
        return len(self.data)

    def __getitem__(self, sl):
        self.seqs.append(sl.start // BODY + 1)
        return self.data[sl]


def test_reference_arrival_order(pkg, dev):
    """scenario_a's chunks as the reference's receive loop would see them:
    every delivered packet (duplicates and corrupted copies included) goes
    into the next ring slot in delivery order, the table points at the first
    accepted copy of each seqNo, and a completed attempt hashes to its
    reassembled buffer."""
    sc = rr.scenario_a(4)
    corpus = rr.corpus(len(sc.chunks))
    packets, lists, bufs, clean = [], [], [], []
    for ci, ch in enumerate(sc.chunks):
        data = corpus[ci * CHUNK:(ci + 1) * CHUNK]
        for attempt in (0, 1):
            rec = Recorded(data)
            att = rr.replay_attempt(rec, sc, ch, attempt)
            assert len(rec.seqs) == att.delivered
            table, count = {}, {}
            for seq in rec.seqs:
                blen = rr.LAST_BODY if seq == NPACK else BODY
                body = bytearray(data[BODY * (seq - 1):BODY * (seq - 1) + blen])
                if attempt == 0:  # the copy on the wire: replay_attempt's corruption rule
                    for s, off, mask, kind in ch.corr:
                        if s == seq and (kind == "D") == (count.get(seq, 0) > 0):
                            body[off] ^= mask
                count[seq] = count.get(seq, 0) + 1
                table.setdefault(seq, (len(packets) * SLOT + HEADER, blen))  # the first copy is the accepted one
                packets.append(bytes(body))
            if att.whole:
                assert sorted(table) == list(range(1, NPACK + 1))
                lists.append([table[s] for s in range(1, NPACK + 1)])
                bufs.append(att.buf)
                clean.append(data)
                break
    assert len(lists) >= 6 and len(packets) > NPACK * len(lists)  # duplicates and dropped attempts lie in the ring too
    ring = pkg.sha1chunk.pinned_alloc(len(packets) * SLOT)
    try:
        ring[:] = GUARD
        for k, body in enumerate(packets):
            ring[k * SLOT + HEADER:k * SLOT + HEADER + len(body)] = np.frombuffer(body, np.uint8)
        want = sha1s(bufs)
        assert np.array_equal(pkg.sha1chunk.hash_gather(ring, lists), want)
        assert pkg.sha1chunk.verify_gather(ring, lists, want).tolist() == [0] * len(lists)
        # a corrupted first copy is what the reference keeps: such a chunk differs from the clean corpus
        assert any(b != c for b, c in zip(bufs, clean))
    finally:
        pkg.sha1chunk.pinned_free(ring)
