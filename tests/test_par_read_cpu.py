"""CPU: the host arithmetic of the file pipeline (csrc/par_read.hpp, which
csrc/rt_file.hip computes with) replayed by tools/par_read_check, a
stand-alone host program: par_reader on real PartPools of width 1..9 against
a fake file (full and short reads, EINTR, a file that ends below `end` in
every part and on part boundaries, a hard error in any part) compared with a
sequential read loop; the slot geometry of a size hint; the reduction over a
file's device ranges.  Plain, under AddressSanitizer + UBSan, and under
ThreadSanitizer (the parts run on the pool's threads)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "congestion-control-with-bittorren_amd")


def test_par_read_model():
    subprocess.run(["make", "-s", "-C", PKG_DIR, "../tools/par_read_check"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "par_read_check")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "par_read_check: ok" in r.stdout


def test_par_read_model_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", PKG_DIR, "par-read-check-asan"], capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "par_read_check: ok" in r.stdout


def test_par_read_model_under_tsan():
    import pytest
    r = subprocess.run(["make", "-s", "-C", PKG_DIR, "par-read-check-tsan"], capture_output=True, text=True,
                       timeout=240)
    if r.returncode != 0 and "par_read_check" not in r.stdout + r.stderr and "tsan" in r.stderr.lower():
        pytest.skip("ThreadSanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "par_read_check: ok" in r.stdout
