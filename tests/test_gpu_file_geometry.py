"""The file pipeline (csrc/rt_file.hip: sha1chunk_hash_fd, make_chunks, the
make-chunks CLI, the master index of verify_chunk_hash) in the geometries
users run it in: reads split over several pread threads, the slot size chosen
from the file's size, rings of 2, 3 and 8 slots, a whole-slot H2D piece, a
file shared by three devices.

The other file tests of the suite set 16 MiB slots and 4 MiB pieces or hash
files of at most 9 chunks, so every read they make is below the 8 MiB at which
par_reader (csrc/par_read.hpp) starts a second part: T = 1 throughout.  Each
scenario here is the smallest that reaches its path, and asserts that it did,
on the backend's diagnostics entry point s1be_file_read_stats (reader calls,
calls split over more than one part, the largest part count, parts that came
up short): a scenario that silently stayed at T = 1 fails.  The expected
counters come from a replay of the pipeline's read loop (_replay), whose part
counts are also written out per scenario as the table below has them.

The geometry is read once per process, so each scenario runs in a fresh
child, whose assertions are the test.  Every digest is compared with hashlib
(computed once per file), and the fd must end at the end of the file.  No
file changes while it is hashed: short parts are 0 everywhere (the shrunken-
file branches are covered by tools/par_read_check on the CPU only).

  A     no STREAM_* / READ_THREADS variable, 200 MiB + 12345 B: slots of 67 MiB
        by the spread rule, 3 fills, 64 MiB reads split 8 ways; through the
        library, through the library with the CLI's own 128 MiB setting, and
        through the CLI
  B     2 slots of 32 MiB, whole-slot pieces, 3 read threads, 147 MiB + 4321 B:
        5 fills, T = 3 with parts of 11184811 B (unaligned pread boundaries),
        the 19 MiB tail with T = 2
  C     8 slots of 16 MiB, 16 read threads, 160 MiB + 777 B: 11 fills (the ring
        wraps), T = 2, the 777-byte last read T = 1
  D     B's file from offset 512 KiB + 5, 32 MiB slots, 8 threads: T = 4 from
        an unaligned position
  E     D's settings over three (virtual) devices: each 49 MiB range read with
        T = 4 then T = 2, digests in file order
  F     B with one read thread: the control, no call split
  G     a 70 MiB + 999 B master file through verify_chunk_hash: the index is
        built through the split reader (T = 4), every chunk verifies, the
        zero-padded last one too, and a wrong hash exits 255
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import _run_verify, verify_driver  # noqa: F401 -- G's C driver and its fixture, as they stand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
PKG_DIR = os.path.join(ROOT, "congestion-control-with-bittorren_amd")
L512 = 524288
MiB = 1 << 20
FILL = 0xAA
SKIP = L512 + 5
MIN_PIECE = 8 * MiB  # csrc/par_read.hpp kMinPiece

gpu = pytest.mark.gpu  # every scenario; the replay of the table needs no device

FILES = {"a": 200 * MiB + 12345, "b": 147 * MiB + 4321, "c": 160 * MiB + 777, "g": 70 * MiB + 999}

# Every variable that shapes the pipeline; a scenario's child gets exactly
# the ones it names.
KNOBS = ("SHA1CHUNK_STREAM_SLOTS", "SHA1CHUNK_STREAM_SLOT_MIB", "SHA1CHUNK_STREAM_PIECE_MIB",
         "SHA1CHUNK_READ_THREADS", "SHA1CHUNK_VIRTUAL_DEVICES", "SHA1CHUNK_FILE_DEVICES",
         "SHA1CHUNK_MASTER_INDEX", "SHA1CHUNK_MASTER_SETTLE_MS")
_B = {"SHA1CHUNK_STREAM_SLOTS": "2", "SHA1CHUNK_STREAM_SLOT_MIB": "32", "SHA1CHUNK_STREAM_PIECE_MIB": "0",
      "SHA1CHUNK_READ_THREADS": "3"}
_D = {"SHA1CHUNK_STREAM_SLOT_MIB": "32", "SHA1CHUNK_STREAM_PIECE_MIB": "0"}
# parts: the part count T of every read that finds bytes, in order (per
# device for E), as the table above states them.
SCENARIOS = {
    "A": dict(env={}, file="a", skip=0, parts=[[8, 1, 8, 1, 8, 1]], fills=3, slot_mib=67),
    "A_cli_setting": dict(env={"SHA1CHUNK_STREAM_SLOT_MIB": "128"}, file="a", skip=0, parts=[[8, 1, 8, 1, 8, 1]],
                          fills=3, slot_mib=67),
    "B": dict(env=_B, file="b", skip=0, parts=[[3, 3, 3, 3, 2]], fills=5, slot_mib=32),
    "C": dict(env={"SHA1CHUNK_STREAM_SLOTS": "8", "SHA1CHUNK_STREAM_SLOT_MIB": "16",
                   "SHA1CHUNK_STREAM_PIECE_MIB": "16", "SHA1CHUNK_READ_THREADS": "16"},
              file="c", skip=0, parts=[[2] * 10 + [1]], fills=11, slot_mib=16),
    "D": dict(env=_D, file="b", skip=SKIP, parts=[[4, 4, 4, 4, 2]], fills=5, slot_mib=32),
    "E": dict(env=dict(_D, SHA1CHUNK_VIRTUAL_DEVICES="3", SHA1CHUNK_FILE_DEVICES="all"), file="b", skip=0,
              parts=[[4, 2]] * 3, fills=2, slot_mib=32),
    "F": dict(env=dict(_B, SHA1CHUNK_READ_THREADS="1"), file="b", skip=0, parts=[[1] * 5], fills=5, slot_mib=32),
    "G": dict(env=dict(_D, SHA1CHUNK_MASTER_SETTLE_MS="0", SHA1CHUNK_MASTER_INDEX="1"), file="g", skip=0,
              parts=[[4, 4, 1]], fills=3, slot_mib=32),
}


def _replay(nbytes: int, env: dict):
    """The read loop of hash_stream_sized over a regular file of nbytes with
    the environment `env`: (slot bytes, fills, the part count of every read
    that finds bytes, reader calls)."""
    nslots = min(8, max(2, int(env.get("SHA1CHUNK_STREAM_SLOTS", 3))))
    slot = min(1024, max(16, int(env.get("SHA1CHUNK_STREAM_SLOT_MIB", 512)))) * MiB
    piece = max(0, int(env.get("SHA1CHUNK_STREAM_PIECE_MIB", 64))) * MiB
    threads = max(1, int(env.get("SHA1CHUNK_READ_THREADS", 8)))
    up = lambda x: -(-x // L512) * L512
    if nbytes:
        slot = min(slot, up(nbytes), max(64 * MiB, up(nbytes // nslots)))
    piece = piece or slot
    pos = calls = fills = 0
    parts = []
    eof = False
    while not eof:
        got = 0
        while got < slot:
            calls += 1
            want = min(piece, slot - got, nbytes - pos)
            if want == 0:
                eof = True
                break
            parts.append(max(1, min(threads, want // MIN_PIECE)))
            got += want
            pos += want
        fills += got > 0
    return slot, fills, parts, calls


def _device_ranges(nbytes: int, nd: int):
    chunks = -(-nbytes // L512)
    return [min(nbytes, chunks * (g + 1) // nd * L512) - chunks * g // nd * L512 for g in range(nd)]


def _expected(name: str):
    """(calls, split calls, largest part count, short parts) of a scenario,
    from the replay -- which must agree with the scenario's own table row."""
    sc = SCENARIOS[name]
    nbytes = FILES[sc["file"]] - sc["skip"]
    nd = int(sc["env"].get("SHA1CHUNK_VIRTUAL_DEVICES", 1))
    runs = [_replay(n, sc["env"]) for n in _device_ranges(nbytes, nd)]
    assert [r[2] for r in runs] == sc["parts"], (name, [r[2] for r in runs])
    assert all(r[0] == sc["slot_mib"] * MiB and r[1] == sc["fills"] for r in runs), (name, runs)
    flat = [t for r in runs for t in r[2]]
    return [sum(r[3] for r in runs), sum(t > 1 for t in flat), max(flat), 0]


def test_replay_matches_the_table():
    """The scenarios reach what their rows claim, by the replay alone (this
    test needs no device): slot sizes, fills and every read's T."""
    want = {"A": [7, 3, 8, 0], "A_cli_setting": [7, 3, 8, 0], "B": [6, 5, 3, 0], "C": [12, 10, 2, 0],
            "D": [6, 5, 4, 0], "E": [9, 6, 4, 0], "F": [6, 0, 1, 0], "G": [4, 2, 4, 0]}
    assert {k: _expected(k) for k in SCENARIOS} == want
    # B's parts of a 32 MiB read over three threads
    assert -(-32 * MiB // 3) == 11184811
    # E: 295 chunks over three devices
    assert _device_ranges(FILES["b"], 3) == [49 * MiB, 49 * MiB, 49 * MiB + 4321]


# --------------------------------------------------------------- the files --
def _digests(data: bytes, start: int) -> bytes:
    return b"".join(hashlib.sha1(data[i:i + L512]).digest() for i in range(start, len(data), L512))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> path of a file of FILES[name] random bytes, written on first
    use with its chunk digests next to it (<path>.sha1 from offset 0,
    <path>.skip.sha1 from SKIP); removed after the module."""
    d = tmp_path_factory.mktemp("geometry")
    made = {}

    def get(name: str) -> str:
        if name not in made:
            path = str(d / (name + ".bin"))
            data = np.random.default_rng(len(name) + FILES[name]).bytes(FILES[name])
            with open(path, "wb") as f:
                f.write(data)
            with open(path + ".sha1", "wb") as f:
                f.write(_digests(data, 0))
            with open(path + ".skip.sha1", "wb") as f:
                f.write(_digests(data, SKIP))
            made[name] = path
        return made[name]

    yield get
    for path in made.values():
        for p in (path, path + ".sha1", path + ".skip.sha1"):
            os.unlink(p)


def _want(path: str, skip: int) -> list:
    raw = open(path + (".skip.sha1" if skip else ".sha1"), "rb").read()
    return [raw[i:i + 20] for i in range(0, len(raw), 20)]


# --------------------------------------------------------------- the child --
def _read_stats(reset: bool = False) -> list:
    lib = os.environ.get("SHA1CHUNK_LIB")
    path = os.environ.get("SHA1CHUNK_BACKEND") or os.path.join(
        os.path.dirname(os.path.abspath(lib)) if lib else PKG_DIR, "libsha1chunk_hip.so")
    be = C.CDLL(path)
    be.s1be_file_read_stats.restype = None
    be.s1be_file_read_stats.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    out = (C.c_uint64 * 4)()
    be.s1be_file_read_stats(out, int(reset))
    return list(out)


def _child_hash_fd(m, name: str, path: str):
    sc = SCENARIOS[name]
    for k in KNOBS:
        assert os.environ.get(k) == sc["env"].get(k), k
    want = _want(path, sc["skip"])
    size = os.path.getsize(path)
    assert size == FILES[sc["file"]] and len(want) == -(-(size - sc["skip"]) // L512)
    m.set_device(0)
    assert _read_stats(reset=True)[3] == 0 and _read_stats() == [0, 0, 0, 0]
    k = len(want)
    out = np.full((k + 1, 20), FILL, np.uint8)
    total = C.c_size_t(1 << 40)
    with open(path, "rb") as f:
        fd = f.fileno()
        os.lseek(fd, sc["skip"], os.SEEK_SET)
        n = m.lib().sha1chunk_hash_fd(fd, out.ctypes.data_as(C.POINTER(C.c_uint8)), k + 1, C.byref(total))
        assert n == k and total.value == k, (n, total.value, m.lib().sha1chunk_last_error())
        assert os.lseek(fd, 0, os.SEEK_CUR) == size, "fd not left at the end of the file"
    wrong = [i for i in range(k) if out[i].tobytes() != want[i]]
    assert not wrong, f"{len(wrong)} of {k} digests differ from hashlib, first at chunk {wrong[0]}"
    assert (out[k] == FILL).all(), "a digest row beyond the file's chunks was written"
    stats = _read_stats()
    print("file_read_stats", name, stats)
    assert stats == _expected(name), (stats, _expected(name))


def _child_master(m, name: str, path: str):
    """verify_chunk_hash in this process: the second call against one file
    builds the index through sha1chunk_hash_fd; a mismatch would exit(-1)."""
    sc = SCENARIOS[name]
    for k in KNOBS:
        assert os.environ.get(k) == sc["env"].get(k), k
    want = _want(path, 0)
    m.set_device(0)
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.ftell.argtypes = [C.c_void_p]
    libc.ftell.restype = C.c_long
    fp = libc.fopen(path.encode(), b"r")
    assert fp
    _read_stats(reset=True)
    m.lib().verify_chunk_hash(fp, want[3].hex().encode(), 3)  # per call: the index is built on the second
    assert _read_stats() == [0, 0, 0, 0]
    for idx in (7, 0, len(want) - 2, 64):
        m.lib().verify_chunk_hash(fp, want[idx].hex().encode(), idx)
        assert libc.ftell(fp) == (idx + 1) * L512
    stats = _read_stats()
    print("file_read_stats", name, stats)
    assert stats == _expected(name), (stats, _expected(name))


_CHILD = r"""
import importlib, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
m = importlib.import_module("congestion-control-with-bittorren_amd")
import test_gpu_file_geometry as T
getattr(T, "_child_" + sys.argv[3])(m, sys.argv[4], sys.argv[5])
print("CHILD OK")
"""


def _env(name: str) -> dict:
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(SCENARIOS[name]["env"])
    return env


def _run_child(which: str, name: str, path: str):
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, TESTS, which, name, path], capture_output=True,
                       text=True, env=_env(name), cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]


def _run_cli(name: str, path: str):
    r = subprocess.run([os.path.join(PKG_DIR, "make-chunks"), path], capture_output=True, text=True, env=_env(name),
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == "".join(f"{i} {h.hex()}\n" for i, h in enumerate(_want(path, 0)))


# ----------------------------------------------------------- the scenarios --
@gpu
def test_default_geometry_spreads_over_the_slots(files):
    """A: nothing set.  A 200 MiB + 12345 B file gets three slots of 67 MiB
    (134 chunks: the file's third, rounded up to a chunk), filled once each by
    a 64 MiB read split over 8 threads and a 3 MiB read on one.  Through the
    library, and through the make-chunks CLI, whose output is the "%d %s\n"
    lines of the same digests."""
    path = files("a")
    _run_child("hash_fd", "A", path)
    _run_cli("A", path)


@gpu
def test_cli_slot_setting_gives_the_same_geometry(files):
    """A again with the 128 MiB slots the make-chunks CLI sets for itself
    (whose counters cannot be read from outside): the spread rule still gives
    67 MiB slots, and the library reports the same reads."""
    _run_child("hash_fd", "A_cli_setting", files("a"))


@gpu
def test_two_slot_ring_three_threads_whole_slot_pieces(files):
    """B: SLOTS=2, SLOT_MIB=32, PIECE_MIB=0 (one read and one H2D copy per
    slot), READ_THREADS=3: 147 MiB + 4321 B in 5 fills of a 2-slot ring, each
    32 MiB read cut in parts of 11184811 B at byte offsets that are no
    multiple of anything, the 19 MiB tail in two parts; library and CLI."""
    path = files("b")
    _run_child("hash_fd", "B", path)
    _run_cli("B", path)


@gpu
def test_eight_slot_ring_wraps(files):
    """C: SLOTS=8, SLOT_MIB=16, PIECE_MIB=16, READ_THREADS=16: 160 MiB + 777 B
    in 11 fills, so the 8-slot ring comes round; 16 MiB reads take two parts
    however many threads there are, and the last read is 777 bytes."""
    _run_child("hash_fd", "C", files("c"))


@gpu
def test_split_reads_from_an_unaligned_position(files):
    """D: the fd seeked to 512 KiB + 5 before the call: chunks are cut from
    there, and every part of the 4-way split starts at an odd offset."""
    _run_child("hash_fd", "D", files("b"))


@gpu
def test_split_reads_over_three_devices(files):
    """E: the file's 295 chunks over three logical devices (98, 98 and 99):
    each device's 49 MiB range is a 32 MiB read in 4 parts and a 17 MiB read
    in 2, from its own pool; digests in file order, the fd at the file's
    end; library and CLI."""
    path = files("b")
    _run_child("hash_fd", "E", path)
    _run_cli("E", path)


@gpu
def test_one_read_thread_is_the_control(files):
    """F: B's geometry with READ_THREADS=1: the same digests, no call split."""
    _run_child("hash_fd", "F", files("b"))


@gpu
def test_master_index_is_built_through_the_split_reader(files, verify_driver, monkeypatch):
    """G: verify_chunk_hash against a 70 MiB + 999 B master with 32 MiB
    whole-slot reads.  In a process of its own the second verify builds the
    index through two reads of 4 parts and one of 1; through the C driver of
    test_gpu_parity.py every one of the 141 chunks then verifies, the last
    one zero-padded to CHUNK_LEN, with the stream left after each chunk, and
    one wrong hash served from the index exits 255."""
    path = files("g")
    _run_child("master", "G", path)
    data = open(path, "rb").read()
    n = -(-len(data) // L512)
    data += bytes(n * L512 - len(data))
    hexes = [hashlib.sha1(data[i * L512:(i + 1) * L512]).hexdigest() for i in range(n)]
    assert n == 141 and hexes[-1] != _want(path, 0)[-1].hex()  # the padded digest is another one
    order = [n - 1, 5] + [(37 * i + 11) % n for i in range(n)]  # every chunk, scattered (37 and 141 are coprime)
    assert sorted(set(order)) == list(range(n))
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SCENARIOS["G"]["env"].items():
        monkeypatch.setenv(k, v)
    a = _run_verify(verify_driver, path, [(i, hexes[i]) for i in order], index=True)
    assert a.returncode == 0, a.stderr[-3000:]
    size = FILES["g"]
    want = "".join(f"calculating chunk hash for a chunk of size {L512}\nthe ascii of calculated hash is {hexes[i]}\n"
                   f"ok {i} pos {min((i + 1) * L512, size)}\n" for i in order)
    assert a.stdout == want
    bad = hexes[77][:-1] + ("0" if hexes[77][-1] != "0" else "1")
    c = _run_verify(verify_driver, path, [(3, hexes[3]), (140, hexes[140]), (77, bad)], index=True)
    assert c.returncode == 255, (c.returncode, c.stderr[-2000:])
    assert "Unmatched chunk hashes" in c.stderr and hexes[77] in c.stderr
    assert c.stdout.count("ok ") == 2
