"""CPU: the drop-in boundary -- the C-ABI library builds, loads, and exports
every symbol include/*.h declares; the SHA1Context layout matches the
reference's; host-only logic (hex codec) behaves like chunk.c; without a
device the engine fails loudly instead of falling back to the CPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "congestion-control-with-bittorren_amd")


def _declared_functions():
    names = set()
    for h in ("sha.h", "chunk_hash.h", "sha1chunk.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"typedef[^;]*;", "", text)
        text = re.sub(r"#define[^\n]*", "", text)
        for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text):
            names.add(m.group(1))
    return names


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", PKG_DIR], check=True)
    return os.path.join(PKG_DIR, "libsha1chunk.so")


def test_every_declared_symbol_is_exported(built, pkg):
    declared = _declared_functions()
    assert {"SHA1Init", "SHA1Update", "SHA1Final", "shahash", "make_chunks", "get_chunk_hash",
            "verify_chunk_hash", "binary2hex", "hex2binary", "verify_hash",
            "sha1chunk_hash_batch"} <= declared
    lib = C.CDLL(built)
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, missing
    # the Python mirror binds exactly the declared C ABI
    assert set(pkg.sha1chunk.exported_symbols()) == declared


def test_sha1context_layout_matches_reference(pkg):
    # /root/reference/sha.h:39-52 (no RUNTIME_ENDIAN): 96 bytes
    ctx = pkg.SHA1Context
    assert C.sizeof(ctx) == 96
    assert ctx.totalLength.offset == 0
    assert ctx.hash.offset == 8
    assert ctx.bufferLength.offset == 28
    assert ctx.buffer.offset == 32


def test_sha_h_layout_compiles_to_96_bytes(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include "sha.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(SHA1Context) == 96, "size");\n'
                   '_Static_assert(offsetof(SHA1Context, hash) == 8, "hash");\n'
                   '_Static_assert(offsetof(SHA1Context, bufferLength) == 28, "len");\n'
                   '_Static_assert(offsetof(SHA1Context, buffer) == 32, "buf");\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "a.out")], check=True)


def test_hex_codec_matches_chunk_c(pkg):
    raw = bytes(range(0, 250, 13))
    h = pkg.binary2hex(raw)
    assert h == raw.hex()  # "%.2x" lowercase, chunk.c:60
    assert pkg.hex2binary(h) == raw
    assert pkg.hex2binary(h.upper()) == raw  # toupper in _hex2binary, chunk.c:68-72


def test_reference_style_caller_compiles_against_headers(tmp_path, built):
    """A caller written against the reference's API links as a drop-in."""
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include <stdio.h>
#include "sha.h"
#include "chunk_hash.h"
int main(void) {
    uint8_t h[SHA1_HASH_SIZE]; char a[41];
    SHA1Context c; SHA1Init(&c); SHA1Update(&c, "abc", 3); SHA1Final(&c, h);
    hex2ascii(h, SHA1_HASH_SIZE, a); puts(a);
    shahash((uint8_t *)"dash", 4, h); binary2hex(h, 20, a); puts(a);
    return 0;
}''')
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", PKG_DIR, "-lsha1chunk", f"-Wl,-rpath,{PKG_DIR}"], check=True)
    assert exe.exists()


def _has_device(pkg):
    try:
        return pkg.device_count() > 0
    except Exception:
        return False


def test_no_device_fails_loudly(pkg, built):
    if _has_device(pkg):
        pytest.skip("a device is present")
    with pytest.raises(pkg.Sha1ChunkError) as ei:
        pkg.shahash(b"abc")
    assert ei.value.code == pkg.sha1chunk.ENODEV
    # the reference-signature C entry points exit(-1) with a message
    r = subprocess.run([os.path.join(PKG_DIR, "make-chunks"), os.path.join(ROOT, "tests/golden/C.tar.gz")],
                       capture_output=True, text=True)
    assert r.returncode == 255
    assert "no HIP device" in r.stderr
    assert r.stdout == ""


def test_verify_queue_without_device_fails_loudly(pkg):
    if _has_device(pkg):
        pytest.skip("a device is present")
    with pytest.raises(pkg.Sha1ChunkError):
        pkg.VerifyQueue(batch=16)


def test_receive_cpus_checks_its_mask(pkg, built):
    """sha1chunk_receive_cpus (include/sha1chunk.h): a NULL or short mask is
    refused before any device work; without a device it fails loudly."""
    L = pkg.sha1chunk.lib()
    doms = C.c_uint(7)
    assert L.sha1chunk_receive_cpus(0, 0, None, 128, C.byref(doms)) == pkg.sha1chunk.EINVAL
    short = (C.c_uint8 * 64)()
    assert L.sha1chunk_receive_cpus(0, 0, short, 64, C.byref(doms)) == pkg.sha1chunk.EINVAL
    assert b"cpu_set_t" in L.sha1chunk_last_error()
    assert doms.value == 7  # untouched on failure
    if not _has_device(pkg):
        with pytest.raises(pkg.Sha1ChunkError) as ei:
            pkg.sha1chunk.receive_cpus(0, 0)
        assert ei.value.code == pkg.sha1chunk.ENODEV


def test_python_mirror_names(pkg):
    for name in ("shahash", "binary2hex", "hex2binary", "make_chunks", "get_chunk_hash",
                 "verify_hash", "SHA1"):
        assert hasattr(pkg, name)


def test_product_does_not_link_the_oracle(built):
    out = subprocess.run(["ldd", built], capture_output=True, text=True).stdout
    assert "oracle" not in out and "sharef" not in out
    syms = subprocess.run(["nm", "-D", built], capture_output=True, text=True).stdout
    assert "oracle_" not in syms and "ref_" not in syms


def test_front_end_links_libc_only(built):
    """libsha1chunk.so -- what the peer and make-chunks link -- needs no HIP:
    it loads libsha1chunk_hip.so from its own directory on the first call
    that needs the GPU, so host-only processes never pay HIP's start-up
    (VERDICT r3 next #5).  The backend exports only its s1be_* entry points
    to the front end, none of the reference's or the batch API's names."""
    out = subprocess.run(["ldd", built], capture_output=True, text=True).stdout
    assert "amdhip64" not in out and "libstdc++" not in out, out
    backend = os.path.join(PKG_DIR, "libsha1chunk_hip.so")
    assert os.path.exists(backend)
    assert "amdhip64" in subprocess.run(["ldd", backend], capture_output=True, text=True).stdout
    nm = subprocess.run(["nm", "-D", "--defined-only", backend], capture_output=True, text=True).stdout
    syms = nm.split()
    assert not [s for s in syms if s.startswith("sha1chunk_") or s in ("shahash", "SHA1Init")]
    assert "s1be_hash_batch" in syms
    assert "s1be_sort_order_async" in syms  # diagnostics for tests/test_gpu_sort.py
    assert "s1be_file_read_stats" in syms  # diagnostics for tests/test_gpu_file_geometry.py
    assert "s1be_launch_stats" in syms  # diagnostics for tests/launch_stats.py
    front = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True).stdout
    assert "file_read_stats" not in front and "launch_stats" not in front  # no front-end symbol
    # every defined dynamic symbol is an entry point (csrc/backend.map): no
    # launcher, kernel stub, class or template instantiation leaks out
    names = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    leaked = [n for n in names if not n.startswith("s1be_")]
    assert names and not leaked, leaked


def test_missing_backend_fails_loudly(tmp_path, built):
    """Without the backend library the front end fails every device call with
    ENODEV and the loader's message (no CPU fallback)."""
    code = ("import ctypes, sys\n"
            "lib = ctypes.CDLL(sys.argv[1])\n"
            "lib.sha1chunk_last_error.restype = ctypes.c_char_p\n"
            "off = (ctypes.c_uint64 * 1)(0); ln = (ctypes.c_uint32 * 1)(3)\n"
            "out = ctypes.create_string_buffer(20)\n"
            "print(lib.sha1chunk_hash_batch(b'abc', off, ln, ctypes.c_size_t(1), out, 0))\n"
            "print(lib.sha1chunk_last_error().decode())\n")
    env = dict(os.environ, SHA1CHUNK_BACKEND=str(tmp_path / "nope.so"))
    r = subprocess.run(["python3", "-c", code, built], capture_output=True, text=True, env=env,
                       timeout=60)
    rc, msg = r.stdout.split("\n", 1)
    assert rc == "-2" and "HIP backend not loaded" in msg, r.stdout
