"""The reference's own reassembly under the scenarios the GPU tests use
(tests/test_gpu_reassembly.py), without a device.

oracle/_ref/reassembly_ref is oracle/reassembly_driver.c built with
-DRSM_REFERENCE_ONLY and linked with the whole unmodified reference, its
chunk.c and sha.c included, and without the library (the library's host path
is no CPU fallback: without a device every call fails, test_host_small.py::
test_knob_is_not_a_fallback).  Mode `plain` is then the reference as it
stands: the Malloc'ed session buffer filled by cumulative_ack /
copy_recv_packet_2_buf, verify_hash at the short last packet, and
copy_chunk_2_job_buf on a match.

This pins the scenario generator, the Python replay (reassembly_replay.py)
and the inputs: the expected verdicts come from hashlib over the replayed
buffers and must be what the reference alone decides."""
import hashlib
import os

import pytest

import reassembly_replay as R

pytestmark = pytest.mark.skipif(not os.path.exists(R.REF_DRIVER),
                                reason="oracle/_ref/reassembly_ref is not built (no reference sources)")


@pytest.fixture(scope="module")
def data():
    return R.corpus(8)


def _run(tmp_path, data, sc):
    paths = R.write_inputs(tmp_path, data, sc)
    rc, lines, err = R.run_driver(R.REF_DRIVER, "plain", paths, dict(os.environ), timeout=120)
    return R.check_run("plain", data, sc, paths, rc, lines, err)


@pytest.mark.parametrize("which", ["a", "b"])
def test_reference_reassembly_matches_replay(tmp_path, data, which):
    """Dumps equal the replay byte for byte, verdicts equal hashlib's, the job
    buffers equal the data file (check_run), under 4 interleaved sessions."""
    sc = (R.scenario_a if which == "a" else R.scenario_b)(4)
    info = _run(tmp_path, data, sc)
    exp = info["_expected"]
    # the scenario does what it is for: out-of-order copies, in-window
    # duplicates, strays, and windows that slide by more than one packet
    assert info["copied_dups"] > 100 and info["strays"] > 10
    jumps = set()
    for a in exp.attempts.values():
        acked = [m // R.BODY for m in a.marks if m < R.CHUNK_LEN]
        jumps |= {y - x for x, y in zip([0] + acked, acked)}
    assert 1 in jumps and max(jumps) == 8, jumps
    assert sum(1 for a in exp.attempts.values() for m in a.marks if m % 64 == 0 and m < R.CHUNK_LEN) < \
        sum(len(a.marks) for a in exp.attempts.values()) / 8


def test_edge_offsets_each_reject_their_chunk(tmp_path, data):
    """Every edge position, flipped in a first copy, turns its chunk's
    verdict to 1, and the clean re-GET verifies."""
    seen = set()
    for sc in (R.scenario_a(4), R.scenario_b(4)):
        exp = R.expected_run(data, sc, "plain")
        for c, ch in enumerate(sc.chunks):
            firsts = [(s - 1) * R.BODY + o for s, o, m, k in ch.corr if k == "F" and m]
            if firsts and not ch.early:
                assert len(firsts) == 1
                assert exp.results[c, 0][0] == 1 and exp.results[c, 1][0] == 0
                seen.add(firsts[0])
    assert seen >= set(R.EDGE_OFFSETS), set(R.EDGE_OFFSETS) - seen


def test_corrupted_duplicate_is_dropped_and_corrupted_first_copy_sticks(tmp_path, data):
    sc = R.scenario_a(4)
    info = _run(tmp_path, data, sc)
    exp = info["_expected"]
    # chunk 5: only duplicate copies are corrupted, each was delivered: verdict 0 at once
    a = exp.attempts[5, 0]
    for s, _, _, kind in sc.chunks[5].corr:
        assert kind == "D" and a.dup_copies.get(s, 0) >= 1
    assert exp.results[5, 0][0] == 0 and (5, 1) not in exp.results
    # chunk 6: the first copy is corrupted and a clean duplicate follows: still 1
    seq = sc.chunks[6].corr[0][0]
    assert exp.attempts[6, 0].dup_copies.get(seq, 0) >= 1
    assert exp.results[6, 0][0] == 1 and exp.results[6, 1][0] == 0


def test_short_last_packet_above_a_hole(tmp_path, data):
    """packet_handler.c:469 completes the chunk at the short datagram: packet
    353 is still missing, the buffer holds the 0xA5 fill there, the reference
    rejects it and the re-GET verifies; the progressive modes drop it."""
    sc = R.scenario_a(4)
    for mode in ("plain", "pv"):
        exp = R.expected_run(data, sc, mode)
        for c in (4, 7):
            a = exp.attempts[c, 0]
            assert not a.whole and 346 <= a.acked < 353
            assert a.buf[352 * R.BODY:353 * R.BODY] == b"\xa5" * R.BODY
            assert a.buf[353 * R.BODY:] == data[c * R.CHUNK_LEN + 353 * R.BODY:(c + 1) * R.CHUNK_LEN]
            if mode == "plain":
                assert exp.results[c, 0][0] == 1 and exp.results[c, 1][0] == 0
            else:
                assert (c, 0) in exp.drops and (c, 0) not in exp.results and exp.results[c, 1][0] == 0


def test_replay_is_a_pure_function_of_the_seed(data):
    sc = R.scenario_b(4)
    chunk = data[:R.CHUNK_LEN]
    one = R.replay_attempt(chunk, sc, sc.chunks[0], 0)
    assert R.replay_attempt(chunk, sc, sc.chunks[0], 0).buf == one.buf
    # other interleaving parameters leave the buffer alone; another attempt is another order
    assert R.replay_attempt(chunk, R.scenario_b(1, gseed=9, subset=100), sc.chunks[0], 0).buf == one.buf
    assert R.replay_attempt(chunk, sc, sc.chunks[0], 1).delivered != one.delivered
    assert hashlib.sha1(R.replay_attempt(chunk, sc, sc.chunks[0], 1).buf).digest() == hashlib.sha1(chunk).digest()
