"""CPU: the progressive verifier's boundary (sha1chunk_pv_*, include/
sha1chunk.h).  Without a device the object cannot be made and says why --
there is no CPU fallback; the Python mirror and the built library carry
every declared name.  (What it computes: tests/test_gpu_progressive.py.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "congestion-control-with-bittorren_amd")


def _has_device(pkg):
    try:
        return pkg.device_count() > 0
    except Exception:
        return False


def _declared_pv_names():
    text = open(os.path.join(ROOT, "include", "sha1chunk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sha1chunk_pv_[a-z_]+)\s*\(", text)))


def test_create_without_device_fails_loudly(pkg):
    L = pkg.lib()
    p = L.sha1chunk_pv_create(4, 4096)
    if _has_device(pkg):
        assert p, L.sha1chunk_last_error()
        L.sha1chunk_pv_destroy(p)
        return
    assert not p
    assert b"no HIP device" in L.sha1chunk_last_error(), L.sha1chunk_last_error()
    with pytest.raises(pkg.Sha1ChunkError) as ei:
        pkg.ProgressiveVerifier(sessions=4, max_chunk_len=4096)
    assert ei.value.code == pkg.sha1chunk.ENODEV


def test_null_object_is_refused(pkg):
    L = pkg.lib()
    E = pkg.sha1chunk.EINVAL
    buf = (C.c_uint8 * 64)()
    n = C.c_uint32(5)
    assert L.sha1chunk_pv_advance(None, buf, 1) == E
    assert L.sha1chunk_pv_hashed(None, buf, C.byref(n)) == E and n.value == 5
    assert L.sha1chunk_pv_close(None, buf) == E
    assert L.sha1chunk_pv_poll(None, None, None, None, 0, 0) == E
    assert L.sha1chunk_pv_open(None, 1, C.cast(buf, C.POINTER(C.c_uint8)), 0) is None
    assert L.sha1chunk_pv_pending(None) == 0
    L.sha1chunk_pv_destroy(None)
    assert not L.sha1chunk_pv_create(0, 4096)
    assert b"session" in L.sha1chunk_last_error()


def test_python_mirror_exposes_progressive_verifier(pkg):
    assert hasattr(pkg, "ProgressiveVerifier") and "ProgressiveVerifier" in pkg.__all__
    for name in ("open", "advance", "hashed", "poll", "close", "pending", "destroy"):
        assert hasattr(pkg.ProgressiveVerifier, name), name
    assert set(_declared_pv_names()) <= set(pkg.sha1chunk.exported_symbols())


def test_every_declared_pv_name_is_exported():
    names = _declared_pv_names()
    assert names == sorted("sha1chunk_pv_" + n for n in
                           ("create", "open", "advance", "hashed", "poll", "close", "pending", "destroy"))
    subprocess.run(["make", "-s", "-C", PKG_DIR], check=True)
    lib = C.CDLL(os.path.join(PKG_DIR, "libsha1chunk.so"))
    assert not [n for n in names if not hasattr(lib, n)]
    # and the backend carries their s1be_ counterparts, which the front end binds at load
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, "libsha1chunk_hip.so")],
                          capture_output=True, text=True, check=True).stdout.split()
    assert not [n for n in names if n.replace("sha1chunk_", "s1be_") not in syms]
