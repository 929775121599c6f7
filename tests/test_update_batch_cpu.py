"""CPU: the batched SHA1Init / SHA1Update / SHA1Final entry points
(include/sha1chunk.h) without a device -- the names through every layer, the
front end's argument checks, which are made before anything is forwarded, and
the split arithmetic of csrc/update_split.hpp replayed by
tools/update_split_check (plain and under AddressSanitizer + UBSan, a
stand-alone host program)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "congestion-control-with-bittorren_amd")
NAMES = ["init_device_async", "update_device_async", "final_device_async", "update_batch", "final_batch"]
EINVAL, ENODEV, EALIGN = -1, -2, -5
HOST, DEVICE, ALL_DEVICES = 0, 1, 2


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", PKG_DIR], check=True)
    return PKG_DIR


def _dynamic_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_names_through_every_layer(built, pkg):
    header = open(os.path.join(ROOT, "include", "sha1chunk.h")).read()
    assert re.search(r"#define\s+SHA1CHUNK_CONTEXT_BYTES\s+96\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    front = _dynamic_symbols(os.path.join(built, "libsha1chunk.so"))
    back = _dynamic_symbols(os.path.join(built, "libsha1chunk_hip.so"))
    bound = set(pkg.sha1chunk.exported_symbols())
    for name in NAMES:
        assert re.search(r"\bint\s+sha1chunk_%s\s*\(" % name, code), f"sha1chunk_{name} not declared"
        assert f"sha1chunk_{name}" in front, f"libsha1chunk.so lacks sha1chunk_{name}"
        assert f"s1be_{name}" in back, f"libsha1chunk_hip.so lacks s1be_{name}"
        assert f"sha1chunk_{name}" in bound, f"the Python mirror does not bind sha1chunk_{name}"
        assert getattr(pkg.lib(), f"sha1chunk_{name}").argtypes is not None
    assert pkg.sha1chunk.CONTEXT_BYTES == 96 == pkg.sha1chunk.CONTEXT_DTYPE.itemsize == C.sizeof(pkg.SHA1Context)


class Host:
    """A small valid host batch: 4 contexts, 3 entries."""

    def __init__(self, pkg):
        self.L = pkg.lib()
        self.ctx = pkg.sha1chunk.new_contexts(4)
        self.ctx["buffer"] = 0xA5
        self.before = self.ctx.tobytes()
        self.base = np.arange(256, dtype=np.uint8)
        self.off = np.array([0, 10, 100], np.uint64)
        self.len = np.array([10, 90, 156], np.uint32)
        self.dig = np.full(3 * 20, 0xAA, np.uint8)

    def update(self, index=(0, 1, 2), n_contexts=4, n=3, flags=HOST, ctx=True, base=True, off=True, ln=True):
        idx = None if index is None else np.array(index, np.uint32)
        return self.L.sha1chunk_update_batch(self.ctx.ctypes.data if ctx else None, n_contexts,
                                             None if idx is None else idx.ctypes.data,
                                             self.base.ctypes.data if base else None,
                                             self.off.ctypes.data if off else None,
                                             self.len.ctypes.data if ln else None, n, flags)

    def final(self, index=(0, 1, 2), n_contexts=4, n=3, flags=HOST, ctx=True, dig=True):
        idx = None if index is None else np.array(index, np.uint32)
        return self.L.sha1chunk_final_batch(self.ctx.ctypes.data if ctx else None, n_contexts,
                                            None if idx is None else idx.ctypes.data, n,
                                            self.dig.ctypes.data if dig else None, flags)

    def untouched(self):
        return self.ctx.tobytes() == self.before and (self.dig == 0xAA).all()


REFUSED = {
    "update: null contexts": lambda h: h.update(ctx=False),
    "update: null base": lambda h: h.update(base=False),
    "update: null offsets": lambda h: h.update(off=False),
    "update: null lengths": lambda h: h.update(ln=False),
    "update: null contexts, device": lambda h: h.update(ctx=False, flags=DEVICE),
    "update: duplicate index": lambda h: h.update(index=(2, 0, 2)),
    "update: index = n_contexts": lambda h: h.update(index=(0, 4, 1)),
    "update: index 2^32 - 1": lambda h: h.update(index=(0, 1, 0xFFFFFFFF)),
    "update: no index, n > n_contexts": lambda h: h.update(index=None, n_contexts=2),
    "update: ALL_DEVICES": lambda h: h.update(flags=ALL_DEVICES),
    "update: DEVICE | ALL_DEVICES": lambda h: h.update(flags=DEVICE | ALL_DEVICES),
    "update: n = 2^32": lambda h: h.update(n=2 ** 32),
    "final: null contexts": lambda h: h.final(ctx=False),
    "final: duplicate index": lambda h: h.final(index=(1, 1, 0)),
    "final: index = n_contexts": lambda h: h.final(index=(4, 1, 0)),
    "final: ALL_DEVICES": lambda h: h.final(flags=ALL_DEVICES),
    "final: n = 2^32": lambda h: h.final(n=2 ** 32),
}


@pytest.mark.parametrize("row", list(REFUSED))
def test_front_end_refuses_before_forwarding(built, pkg, row):
    h = Host(pkg)
    assert REFUSED[row](h) == EINVAL, pkg.lib().sha1chunk_last_error()
    assert pkg.lib().sha1chunk_last_error() != b""
    assert h.untouched()


def test_device_forms_refuse_null_and_misaligned(built, pkg):
    L = pkg.lib()
    d = np.zeros(256, np.uint8).ctypes.data & ~7  # never dereferenced: every call below is refused first
    assert L.sha1chunk_init_device_async(None, 4, None, 4, None) == EINVAL
    assert L.sha1chunk_update_device_async(None, 4, None, d, d, d, 4, None) == EINVAL
    assert L.sha1chunk_update_device_async(d, 4, None, None, d, d, 4, None) == EINVAL
    assert L.sha1chunk_update_device_async(d, 4, None, d, None, d, 4, None) == EINVAL
    assert L.sha1chunk_update_device_async(d, 4, None, d, d, None, 4, None) == EINVAL
    assert L.sha1chunk_final_device_async(None, 4, None, 4, d, None) == EINVAL
    assert L.sha1chunk_final_device_async(d, 4, None, 4, d + 2, None) == EALIGN
    assert L.sha1chunk_final_batch(d, 4, None, 4, d + 1, DEVICE) == EALIGN
    assert L.sha1chunk_init_device_async(d, 4, None, 2 ** 32 - 1024, None) == EINVAL
    # n == 0 is a successful no-op, whatever the pointers
    assert L.sha1chunk_init_device_async(None, 0, None, 0, None) == 0
    assert L.sha1chunk_update_device_async(None, 0, None, None, None, None, 0, None) == 0
    assert L.sha1chunk_final_device_async(None, 0, None, 0, None, None) == 0
    assert L.sha1chunk_update_batch(None, 0, None, None, None, None, 0, HOST) == 0
    assert L.sha1chunk_final_batch(None, 0, None, 0, None, ALL_DEVICES) == 0


def test_valid_host_call_without_a_device_is_enodev(built, pkg):
    if pkg.device_count() > 0:
        pytest.skip("a device is present: the calls would run")
    h = Host(pkg)
    assert h.update() == ENODEV, pkg.lib().sha1chunk_last_error()
    assert b"device" in pkg.lib().sha1chunk_last_error()
    assert h.update(index=None, n_contexts=3) == ENODEV
    assert h.final() == ENODEV
    assert h.final(dig=False) == ENODEV
    assert h.untouched()


def test_valid_host_call_without_the_backend_is_enodev(tmp_path, built):
    """No CPU fallback: with the backend library missing, the valid calls
    fail with ENODEV and the loader's message, and refused ones are still
    refused first (on any machine: the child never reaches a device)."""
    code = ("import ctypes as C, sys\n"
            "L = C.CDLL(sys.argv[1])\n"
            "L.sha1chunk_last_error.restype = C.c_char_p\n"
            "ctx = C.create_string_buffer(2 * 96); data = C.create_string_buffer(b'x' * 100)\n"
            "off = (C.c_uint64 * 2)(0, 50); ln = (C.c_uint32 * 2)(50, 50); dig = C.create_string_buffer(40)\n"
            "dup = (C.c_uint32 * 2)(1, 1)\n"
            "z = C.c_size_t\n"
            "print(L.sha1chunk_update_batch(ctx, z(2), None, data, off, ln, z(2), 0))\n"
            "print(L.sha1chunk_last_error().decode())\n"
            "print(L.sha1chunk_final_batch(ctx, z(2), None, z(2), dig, 0))\n"
            "print(L.sha1chunk_update_batch(ctx, z(2), dup, data, off, ln, z(2), 0))\n"
            "print(L.sha1chunk_init_device_async(ctx, z(2), None, z(2), None))\n"
            "print(ctx.raw == bytes(192) and dig.raw == bytes(40))\n")
    env = dict(os.environ, SHA1CHUNK_BACKEND=str(tmp_path / "nope.so"))
    r = subprocess.run(["python3", "-c", code, os.path.join(built, "libsha1chunk.so")], capture_output=True, text=True,
                       env=env, timeout=60)
    lines = r.stdout.splitlines()
    assert lines[0] == str(ENODEV) and "HIP backend not loaded" in lines[1], r.stdout + r.stderr
    assert lines[2:] == [str(ENODEV), str(EINVAL), str(ENODEV), "True"], r.stdout + r.stderr


def test_split_arithmetic(built):
    subprocess.run(["make", "-s", "-C", PKG_DIR, "../tools/update_split_check"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "update_split_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "update_split_check: ok" in r.stdout


def test_split_arithmetic_under_sanitizers(built):
    r = subprocess.run(["make", "-s", "-C", PKG_DIR, "split-check-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "update_split_check: ok" in r.stdout
