"""The backend's launch counters (s1be_launch_stats, csrc/rt_device.hip), for
the tests that check which kernel a call launches: a ctypes view of the
libsha1chunk_hip.so that the package loaded.  Not a test module.

The counters are process-wide and count a kernel where its launcher enqueues
it (csrc/sha1_kernels.h LaunchCounter fixes the layout of out[12]):

  [0] lane       [1] fused      [2] unit1     [3] unit4
  [4] unit11_lane    split unit 11, lane-per-chunk producer loads
  [5] unit11_shared  split unit 11, loads shared across the wave
  [6] quad       split unit 416
  [7] study      a shape of the A/B library only
  [8] mixed      [9] sort       the longest-first length sort
  [10] drain     a persistent verify-queue drain
  [11] drain_cus gauge, never reset: CUs the calling thread's device's
                 persistent drains hold now

snapshot() reads them (the gauge included), delta(before) gives what was
launched since `before` as a dict of the eleven counters, and expect(...)
builds the dict a test compares it with, every counter it does not name 0 --
so an assertion on a delta also says that nothing else was launched."""
import ctypes as C
import os

NAMES = ("lane", "fused", "unit1", "unit4", "unit11_lane", "unit11_shared", "quad", "study", "mixed", "sort",
         "drain")
GAUGE = len(NAMES)  # out[11]
# the kernels that hash a batch (everything but the sort and the drain)
HASH = NAMES[:9]
KNOBS = ("SHA1CHUNK_SPLIT_UNIT", "SHA1CHUNK_FORCE_KERNEL", "SHA1CHUNK_MIXED", "SHA1CHUNK_MIXED_PLAN")
PKG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "congestion-control-with-bittorren_amd")

_be = None


def backend() -> C.CDLL:
    """The backend the front end loads: next to SHA1CHUNK_LIB's library (or
    SHA1CHUNK_BACKEND itself), else the package's own."""
    global _be
    if _be is None:
        lib = os.environ.get("SHA1CHUNK_LIB")
        path = os.environ.get("SHA1CHUNK_BACKEND") or os.path.join(
            os.path.dirname(os.path.abspath(lib)) if lib else PKG_DIR, "libsha1chunk_hip.so")
        _be = C.CDLL(path)
        _be.s1be_launch_stats.restype = None
        _be.s1be_launch_stats.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    return _be


def snapshot(reset: bool = False) -> list:
    """The eleven counters and the gauge, as 12 ints."""
    out = (C.c_uint64 * (GAUGE + 1))()
    backend().s1be_launch_stats(out, int(reset))
    return [int(v) for v in out]


def delta(before: list) -> dict:
    """Launches since the snapshot `before`, by counter name."""
    now = snapshot()
    return {k: now[i] - before[i] for i, k in enumerate(NAMES)}


def drain_cus() -> int:
    return snapshot()[GAUGE]


def expect(**counts) -> dict:
    """A whole delta: the named counters, every other one 0."""
    unknown = set(counts) - set(NAMES)
    assert not unknown, unknown
    return {k: counts.get(k, 0) for k in NAMES}


def clear_knobs(monkeypatch, **env):
    """Remove the dispatch knobs from the environment, then set `env`."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
