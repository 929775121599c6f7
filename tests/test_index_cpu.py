"""CPU: the digest index (include/sha1chunk.h, "Digest index") without a device
-- the names through every layer, the front end's refusals, which are made
before the backend is loaded and leave the outputs alone, ENODEV without a
device and without the backend, the chunk-list reader behind has_chunks, and
the index's insert and lookup (csrc/index_map.hpp) run by
tools/index_map_check, plain and under AddressSanitizer + UBSan (a stand-alone
host program)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "congestion-control-with-bittorren_amd")
NAMES = ["index_create", "index_destroy", "index_size", "index_lookup_device_async", "index_lookup", "match_batch",
         "match_fd"]
EINVAL, ENODEV, EALIGN = -1, -2, -5
HOST, DEVICE, ALL_DEVICES = 0, 1, 2
GUARD = 0xA5A5A5A5
CHAIN_SEED = 20261020  # tests/test_gpu_index.py CHAIN_SEED
CHECK_OK = r"index_map_check: \d+ builds, \d+ lookups: ok"


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", PKG_DIR], check=True)
    return PKG_DIR


def _dynamic_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_names_through_every_layer(built, pkg):
    header = open(os.path.join(ROOT, "include", "sha1chunk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    front = _dynamic_symbols(os.path.join(built, "libsha1chunk.so"))
    back = _dynamic_symbols(os.path.join(built, "libsha1chunk_hip.so"))
    bound = set(pkg.sha1chunk.exported_symbols())
    for name in NAMES:
        assert re.search(r"\b(int|long|void|size_t|sha1chunk_index\s*\*)\s*sha1chunk_%s\s*\(" % name, code), \
            f"sha1chunk_{name} not declared"
        assert f"sha1chunk_{name}" in front, f"libsha1chunk.so lacks sha1chunk_{name}"
        assert f"s1be_{name}" in back, f"libsha1chunk_hip.so lacks s1be_{name}"
        assert f"sha1chunk_{name}" in bound, f"the Python mirror does not bind sha1chunk_{name}"
        assert getattr(pkg.lib(), f"sha1chunk_{name}").argtypes is not None
    assert re.search(r"#define\s+SHA1CHUNK_NO_MATCH\s+0xFFFFFFFFu", code)
    assert re.search(r"typedef\s+struct\s+sha1chunk_index\s+sha1chunk_index\s*;", code)
    assert pkg.sha1chunk.NO_MATCH == 0xFFFFFFFF
    # the diagnostics are a backend-only export
    assert "s1be_index_stats" in back
    assert not [s for s in front if "index_stats" in s]
    assert "index_stats" not in header
    for fn in ("lookup", "lookup_device", "match_batch", "match_fd", "size", "close", "__enter__", "__exit__"):
        assert hasattr(pkg.DigestIndex, fn)
    assert callable(pkg.has_chunks)


class Call:
    """Arguments of valid calls, with guard-filled outputs.  The index handle is
    never dereferenced: every call made with it here is refused first."""

    def __init__(self, pkg):
        self.L = pkg.lib()
        self.ix = np.zeros(64, np.uint8).ctypes.data & ~7
        self.keep = np.zeros(64 + 4, np.uint32)
        self.dig = np.arange(4 * 20, dtype=np.uint8)
        self.ids = np.full(4 + 2, GUARD, np.uint32)
        self.base = np.arange(256, dtype=np.uint8)
        self.off = np.array([0, 10, 100, 200], np.uint64)
        self.len = np.array([10, 90, 0, 56], np.uint32)
        self.total = C.c_size_t(77)

    def create(self, dig=True, m=4, flags=HOST, shift=0):
        return self.L.sha1chunk_index_create(self.dig.ctypes.data + shift if dig else None, m, flags)

    def lookup(self, ix=True, dig=True, n=4, ids=True, shift_dig=0, shift_ids=0, device=False):
        a = (self.ix if ix else None, self.dig.ctypes.data + shift_dig if dig else None, n,
             self.ids.ctypes.data + shift_ids if ids else None)
        return self.L.sha1chunk_index_lookup_device_async(*a, None) if device else self.L.sha1chunk_index_lookup(*a)

    def match(self, ix=True, base=True, off=True, ln=True, n=4, ids=True, shift_ids=0, flags=HOST):
        return self.L.sha1chunk_match_batch(self.ix if ix else None, self.base.ctypes.data if base else None,
                                            self.off.ctypes.data if off else None,
                                            self.len.ctypes.data if ln else None, n,
                                            self.ids.ctypes.data + shift_ids if ids else None, flags)

    def match_fd(self, ix=True, ids=True, max_chunks=4, shift_ids=0, fd=-1):
        return self.L.sha1chunk_match_fd(self.ix if ix else None, fd, self.ids.ctypes.data + shift_ids if ids else None,
                                         max_chunks, C.byref(self.total))

    def untouched(self):
        return (self.ids == GUARD).all() and self.total.value == 77


# row -> (call, expected code); create answers NULL (None) instead of a code
REFUSED = {
    "create: null digests": (lambda c: c.create(dig=False), None),
    "create: m = 2^31 + 1": (lambda c: c.create(m=2 ** 31 + 1), None),
    "create: ALL_DEVICES": (lambda c: c.create(flags=ALL_DEVICES), None),
    "create: DEVICE | ALL_DEVICES": (lambda c: c.create(flags=DEVICE | ALL_DEVICES), None),
    "create: unknown flag": (lambda c: c.create(flags=8), None),
    "create: digests at 2 mod 4": (lambda c: c.create(shift=2), None),
    "lookup: null index": (lambda c: c.lookup(ix=False), EINVAL),
    "lookup: null index, n = 0": (lambda c: c.lookup(ix=False, n=0), EINVAL),
    "lookup: null digests": (lambda c: c.lookup(dig=False), EINVAL),
    "lookup: null ids": (lambda c: c.lookup(ids=False), EINVAL),
    "lookup: n = 2^32 - 255": (lambda c: c.lookup(n=2 ** 32 - 255), EINVAL),
    "lookup: n = 2^40": (lambda c: c.lookup(n=2 ** 40), EINVAL),
    "lookup: digests at 1 mod 4": (lambda c: c.lookup(shift_dig=1), EALIGN),
    "lookup: ids at 2 mod 4": (lambda c: c.lookup(shift_ids=2), EALIGN),
    "lookup_device: null index": (lambda c: c.lookup(ix=False, device=True), EINVAL),
    "lookup_device: null digests": (lambda c: c.lookup(dig=False, device=True), EINVAL),
    "lookup_device: null ids": (lambda c: c.lookup(ids=False, device=True), EINVAL),
    "lookup_device: n = 2^32 - 255": (lambda c: c.lookup(n=2 ** 32 - 255, device=True), EINVAL),
    "lookup_device: digests at 2 mod 4": (lambda c: c.lookup(shift_dig=2, device=True), EALIGN),
    "lookup_device: ids at 3 mod 4": (lambda c: c.lookup(shift_ids=3, device=True), EALIGN),
    "match_batch: null index": (lambda c: c.match(ix=False), EINVAL),
    "match_batch: null base": (lambda c: c.match(base=False), EINVAL),
    "match_batch: null offsets": (lambda c: c.match(off=False), EINVAL),
    "match_batch: null lengths": (lambda c: c.match(ln=False), EINVAL),
    "match_batch: null ids": (lambda c: c.match(ids=False), EINVAL),
    "match_batch: null base, device": (lambda c: c.match(base=False, flags=DEVICE), EINVAL),
    "match_batch: ALL_DEVICES": (lambda c: c.match(flags=ALL_DEVICES), EINVAL),
    "match_batch: ALL_DEVICES, n = 0": (lambda c: c.match(flags=ALL_DEVICES, n=0), EINVAL),
    "match_batch: unknown flag": (lambda c: c.match(flags=4), EINVAL),
    "match_batch: n = 2^32 - 1024": (lambda c: c.match(n=2 ** 32 - 1024), EINVAL),
    "match_batch: ids at 2 mod 4": (lambda c: c.match(shift_ids=2), EALIGN),
    "match_fd: null index": (lambda c: c.match_fd(ix=False), EINVAL),
    "match_fd: null ids": (lambda c: c.match_fd(ids=False), EINVAL),
    "match_fd: ids at 1 mod 4": (lambda c: c.match_fd(shift_ids=1), EALIGN),
}


def test_front_end_refuses_before_forwarding(tmp_path, built):
    """One table, in one child process whose backend cannot be loaded: a row
    that was forwarded would answer ENODEV.  Each row leaves the guards intact
    and is followed by the next."""
    code = ("import importlib, sys\n"
            f"sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import test_index_cpu as T\n"
            "pkg = importlib.import_module('congestion-control-with-bittorren_amd')\n"
            "c = T.Call(pkg)\n"
            "for row, (call, want) in T.REFUSED.items():\n"
            "    got = call(c)\n"
            "    err = pkg.lib().sha1chunk_last_error()\n"
            "    assert got == want, (row, got, err)\n"
            "    assert err and b'backend' not in err, (row, err)\n"
            "    assert c.untouched(), row\n"
            "print('rows', len(T.REFUSED))\n")
    env = dict(os.environ, SHA1CHUNK_BACKEND=str(tmp_path / "nope.so"))
    r = subprocess.run(["python3", "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and f"rows {len(REFUSED)}" in r.stdout, r.stdout + r.stderr


def test_no_ops(built, pkg):
    L = pkg.lib()
    L.sha1chunk_index_destroy(None)
    assert L.sha1chunk_index_size(None) == 0


def test_valid_calls_without_a_device_are_enodev(built, pkg):
    if pkg.device_count() > 0:
        pytest.skip("a device is present: the calls would run")
    c = Call(pkg)
    assert c.create() is None
    assert b"device" in pkg.lib().sha1chunk_last_error()
    assert c.create(m=0, dig=False) is None
    with pytest.raises(pkg.Sha1ChunkError) as ei:
        pkg.DigestIndex(np.zeros((3, 20), np.uint8))
    assert ei.value.code == ENODEV
    with pytest.raises(pkg.Sha1ChunkError) as ei:
        pkg.DigestIndex([])
    assert ei.value.code == ENODEV
    # with a handle the calls are forwarded; the device probe then refuses them
    # before the handle is looked at
    assert c.lookup() == ENODEV, pkg.lib().sha1chunk_last_error()
    assert c.lookup(device=True) == ENODEV
    assert c.match() == ENODEV
    assert c.match(flags=DEVICE) == ENODEV
    assert c.match_fd() == ENODEV
    assert c.untouched()


def test_valid_calls_without_the_backend_are_enodev(tmp_path, built):
    """No CPU fallback and no host hash map: with the backend library missing
    the valid calls fail with ENODEV and the loader's message (on any machine:
    the child never reaches a device)."""
    code = ("import ctypes as C, sys\n"
            "L = C.CDLL(sys.argv[1])\n"
            "L.sha1chunk_last_error.restype = C.c_char_p\n"
            "L.sha1chunk_index_create.restype = C.c_void_p\n"
            "L.sha1chunk_match_fd.restype = C.c_long\n"
            "dig = (C.c_uint32 * 10)(); ids = (C.c_uint32 * 2)(7, 7); ix = C.c_void_p(C.addressof(dig))\n"
            "data = C.create_string_buffer(b'x' * 100); off = (C.c_uint64 * 2)(0, 50); ln = (C.c_uint32 * 2)(50, 50)\n"
            "z = C.c_size_t\n"
            "print(L.sha1chunk_index_create(dig, z(2), 0))\n"
            "print(L.sha1chunk_last_error().decode())\n"
            "print(L.sha1chunk_index_create(None, z(0), 0))\n"
            "print(L.sha1chunk_index_lookup(ix, dig, z(2), ids))\n"
            "print(L.sha1chunk_index_lookup_device_async(ix, dig, z(2), ids, None))\n"
            "print(L.sha1chunk_match_batch(ix, data, off, ln, z(2), ids, 0))\n"
            "print(L.sha1chunk_match_batch(ix, data, off, ln, z(2), ids, 2))\n"
            "print(L.sha1chunk_match_fd(ix, 0, ids, z(2), None))\n"
            "print(list(ids))\n")
    env = dict(os.environ, SHA1CHUNK_BACKEND=str(tmp_path / "nope.so"))
    r = subprocess.run(["python3", "-c", code, os.path.join(built, "libsha1chunk.so")], capture_output=True, text=True,
                       env=env, timeout=60)
    lines = r.stdout.splitlines()
    assert lines[0] == "None" and "HIP backend not loaded" in lines[1], r.stdout + r.stderr
    assert lines[2:] == ["None", str(ENODEV), str(ENODEV), str(ENODEV), str(EINVAL), str(ENODEV), "[7, 7]"], \
        r.stdout + r.stderr


def test_read_ids(tmp_path, pkg, golden):
    """chunkfile.read_ids, what has_chunks builds its index from: a plain chunk
    file, CRLF line ends, and the master file whose header carries chunk 0."""
    chunkfile = __import__("importlib").import_module("congestion-control-with-bittorren_amd.chunkfile")
    hashes = golden["fixtures"]["C.chunks_file"]
    plain = tmp_path / "C.chunks"
    plain.write_text("".join(f"{i} {h}\n" for i, h in enumerate(hashes)))
    assert chunkfile.read_ids(plain) == list(enumerate(hashes))
    master = tmp_path / "C.masterchunks"
    master.write_bytes(("\r\n".join([f"File: /tmp/C.tar Chunks:0 {hashes[0]}"] +
                                    [f"{i} {h}" for i, h in enumerate(hashes) if i]) + "\r\n").encode())
    assert chunkfile.read_ids(master) == list(enumerate(hashes))
    has = tmp_path / "B.haschunks"
    has.write_bytes(f"# comment\r\n3 {hashes[3].upper()}\r\n\r\n2 {hashes[2]}\r\nnot a line\r\n".encode())
    assert chunkfile.read_ids(has) == [(3, hashes[3]), (2, hashes[2])]


def _chain_line(out):
    m = re.search(r"chain seed (\d+): prefixes with a home in slots 312\.\.511:([ \d]*); a chain of 200 wraps for:([ \d]*)",
                  out)
    assert m, out
    return int(m.group(1)), m.group(2).split(), m.group(3).split()


def test_index_map(built):
    subprocess.run(["make", "-s", "-C", PKG_DIR, "../tools/index_map_check"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "index_map_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(CHECK_OK, r.stdout)
    # the GPU chain test's seed: at least one of its 32 prefixes has its home in
    # the last 200 of 512 slots, and a chain of 200 from it wraps
    seed, in_last, wraps = _chain_line(r.stdout)
    assert seed == CHAIN_SEED
    assert in_last and wraps and set(wraps) <= set(in_last)
    assert all(0 <= int(k) < 32 for k in in_last)


def test_index_map_under_sanitizers(built):
    r = subprocess.run(["make", "-s", "-C", PKG_DIR, "index-check-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(CHECK_OK, r.stdout)
