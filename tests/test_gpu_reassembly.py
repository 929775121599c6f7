"""The verify queue and the progressive verifier inside the reference's
receive path: oracle/_ref/dropin/reassembly_driver (oracle/reassembly_driver.c)
lets the unmodified reliable_udp.c reassemble 512 KiB chunks -- out of order,
with duplicates, strays, corrupted packets and sessions dropped part-way --
in the library's own buffers, S sessions interleaved, and verifies them
through sha1chunk_vq_submit, reserve/commit/poll/release, sha1chunk_pv_advance
and sha1chunk_burst_advance.

Expected values never come from the library: verdicts and digests are
hashlib's over the Python replay of the schedule (reassembly_replay.py, pinned
against the reference alone by test_reassembly_cpu.py), buffers are the
replay's, job buffers the data file.  check_run() asserts, for every case:
exit status 0 (the driver itself exits non-zero on a library error, on
sha1chunk_pv_hashed() above the stated mark or off a 64-byte boundary, and on
a dropped session's tag coming back), each tag exactly once, verdicts, pv
digests, dumps and job buffers.

Scenarios A and B (reassembly_replay.py) flip one bit at bytes 0, 1483, 1484,
1535, 1536, one byte of packet 177, 523851, 523852 and 524287, each in a
chunk of its own, and each holds two chunks whose short last packet arrives
above a hole (verified with the hole by the queue, dropped and re-opened
under a new tag by the progressive verifier)."""
import os

import pytest

import reassembly_replay as R
from conftest import default_env

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not os.path.exists(R.DRIVER),
                                 reason="oracle/_ref/dropin/reassembly_driver is not built (no reference sources)")]

VQ_CONFIGS = {
    "persistent": {"SHA1CHUNK_VQ_MODE": "persistent"},
    "persistent-nodma": {"SHA1CHUNK_VQ_MODE": "persistent", "SHA1CHUNK_VQ_DMA": "0"},
    "batch": {"SHA1CHUNK_VQ_MODE": "batch"},
}
PV_CONFIGS = {
    "lane-d2": {"SHA1CHUNK_PV_KERNEL": "lane", "SHA1CHUNK_PV_DEPTH": "2"},
    "lane-d8": {"SHA1CHUNK_PV_KERNEL": "lane", "SHA1CHUNK_PV_DEPTH": "8"},
    "shared": {"SHA1CHUNK_PV_KERNEL": "shared"},
}
_KNOBS = [k for cfg in list(VQ_CONFIGS.values()) + list(PV_CONFIGS.values()) for k in cfg] + ["SHA1CHUNK_VQ_RING_MIB"]


@pytest.fixture(scope="module")
def corpora():
    cache = {}

    def get(k):
        if k not in cache:
            cache[k] = R.corpus(k)
        return cache[k]
    return get


def _run(tmp_path, mode, data, sc, env_extra, base=None):
    env = {k: v for k, v in (base or os.environ).items() if k not in _KNOBS}
    env.update(env_extra)
    paths = R.write_inputs(tmp_path, data, sc)
    rc, lines, err = R.run_driver(R.DRIVER, mode, paths, env, timeout=120)
    info = R.check_run(mode, data, sc, paths, rc, lines, err)
    print({k: v for k, v in info.items() if k != "_expected"})
    return info


def test_plain_reference_verify_through_the_library(tmp_path, corpora):
    """Mode plain, default routing: the reference's verify_hash at
    packet_handler.c:472 hashes through the library's host path."""
    _run(tmp_path, "plain", corpora(8), R.scenario_a(4), {}, base=default_env())


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("config", list(VQ_CONFIGS))
@pytest.mark.parametrize("mode", ["submit", "reserve"])
def test_verify_queue(tmp_path, corpora, mode, config, which):
    """S = 4 sessions, K = 8 chunks, corrupted chunks and their re-GETs.  In
    reserve mode the chunks are reassembled in the ring, neighbours filling
    while a committed one is verified and while one verified buffer is kept
    unreleased, and copy_chunk_2_job_buf reads the ring before release()."""
    sc = (R.scenario_a if which == "a" else R.scenario_b)(4)
    info = _run(tmp_path, mode, corpora(8), sc, VQ_CONFIGS[config])
    assert len(info["_expected"].results) > 8  # re-GETs happened
    if mode == "reserve":
        assert info["stability_writes"] > 0


def test_reserve_ring_reuse(tmp_path, corpora):
    """The smallest ring (SHA1CHUNK_VQ_RING_MIB=1 is raised to two groups of
    64 regions of 512 KiB: 128 regions) and K = 3 x 128 chunks: every region
    is handed out three times while its neighbours are still filling, and a
    verified, polled and unreleased buffer is kept until reserve() finds no
    room without it (ring_full), then copied to the job buffer."""
    regions = 2 * 64
    k = 3 * regions
    sc = R.scenario_many(4, k, reorder=25, stray=1)
    info = _run(tmp_path, "reserve", corpora(k), sc,
                dict(VQ_CONFIGS["persistent"], SHA1CHUNK_VQ_RING_MIB="1"))
    assert info["ring_full"] >= 2, info["ring_full"]


@pytest.mark.parametrize("sessions", [1, 5, 20])
@pytest.mark.parametrize("config", list(PV_CONFIGS))
@pytest.mark.parametrize("mode", ["pv", "pv-burst"])
def test_progressive(tmp_path, corpora, mode, config, sessions):
    """The mark is min(CHUNK_LEN, 1484 x last_packet_acked) as cumulative_ack
    moves it, 1 to 8 packets at a time; everything above it is 0xA5 or being
    written.  Every case holds at least two short_last_early chunks (close()
    with launches in flight, re-open under a new tag), so each kernel has its
    case of them.  K = 8 chunks, and 20 with 20 sessions, so that 20 are open
    at once.  After 15 % of the advances the driver waits for the device to
    reach the mark: the kernel's next read then starts right below a packet
    that has not arrived (0xA5), whatever the two sides' speeds."""
    if sessions == 1:
        sc = R.scenario_a(1, subset=100)
    elif sessions == 5:
        sc = R.scenario_b(5)
    else:
        sc = R.scenario_many(20, 20)
    info = _run(tmp_path, mode, corpora(len(sc.chunks)), sc, PV_CONFIGS[config])
    exp = info["_expected"]
    assert len(exp.drops) >= 2 and info["syncs"] > 20
    assert info["kernel"] == (2 if config == "shared" else 1)
    assert info["launches_shared"] == (info["launches"] if config == "shared" else 0)
    if config != "shared":
        assert info["depth"] == int(PV_CONFIGS[config]["SHA1CHUNK_PV_DEPTH"])


def test_burst_auto_routes_both_kernels(tmp_path, corpora):
    """65 sessions served every round, mostly in order: rounds in which at
    least 64 of them gained a whole block take the shared-load kernel, the
    thinner ones (the start of the re-GETs, the tail) the lane kernel."""
    sc = R.scenario_many(65, 65, subset=100, reorder=4, stray=0)
    info = _run(tmp_path, "pv-burst", corpora(65), sc, {"SHA1CHUNK_PV_KERNEL": "auto"})
    assert info["kernel"] == 0
    assert info["launches_shared"] > 0 and info["launches"] > info["launches_shared"], info
