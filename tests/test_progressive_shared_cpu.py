"""CPU: the boundary of the many-session additions to the progressive
verifier (include/sha1chunk.h: sha1chunk_burst_advance,
sha1chunk_progress_stats) and the host check of the shared kernel's address
map (tools/pv_shared_map_check.cc over csrc/pv_shared_map.hpp).  What the
kernel computes: tests/test_gpu_progressive_shared.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "congestion-control-with-bittorren_amd")
NAMES = ("sha1chunk_burst_advance", "sha1chunk_progress_stats")


def test_new_names_are_declared_exported_and_bound(pkg):
    text = open(os.path.join(ROOT, "include", "sha1chunk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "sha1chunk_progress_stats_t" in text
    subprocess.run(["make", "-s", "-C", PKG_DIR], check=True)
    lib = C.CDLL(os.path.join(PKG_DIR, "libsha1chunk.so"))
    assert not [n for n in NAMES if not hasattr(lib, n)]
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, "libsha1chunk_hip.so")],
                          capture_output=True, text=True, check=True).stdout.split()
    assert not [n for n in NAMES if n.replace("sha1chunk_", "s1be_") not in syms]
    assert set(NAMES) <= set(pkg.sha1chunk.exported_symbols())
    # the Python mirror of the struct is the C one: 4 x 8 + 2 x 4 bytes
    assert C.sizeof(pkg.sha1chunk.ProgressStats) == 40


def test_null_object_is_refused(pkg):
    L = pkg.lib()
    E = pkg.sha1chunk.EINVAL
    buf = (C.c_uint8 * 64)()
    bufs = (C.c_void_p * 1)(C.addressof(buf))
    marks = (C.c_uint32 * 1)(1)
    applied = C.c_size_t(7)
    assert L.sha1chunk_burst_advance(None, bufs, marks, 1, C.byref(applied)) == E
    assert applied.value == 0
    assert L.sha1chunk_burst_advance(None, None, None, 0, None) == E
    st = pkg.sha1chunk.ProgressStats()
    st.launches = 5
    assert L.sha1chunk_progress_stats(None, C.byref(st), C.sizeof(st)) == E and st.launches == 5
    assert b"null" in L.sha1chunk_last_error()


def test_python_mirror_has_the_burst_form(pkg):
    for name in ("advance_many", "stats"):
        assert callable(getattr(pkg.ProgressiveVerifier, name, None)), name


def test_address_map_program_builds_and_passes():
    exe = os.path.join(ROOT, "tools", "pv_shared_map_check")
    subprocess.run(["make", "-s", "-C", PKG_DIR, "../tools/pv_shared_map_check"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
